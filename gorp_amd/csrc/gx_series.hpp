// gx_series.hpp -- the rule of gx_group_series, once: plain C++ for the host (g++ alone: tests/cpp/series_test.cpp) and for the kernels
// (gx_series.hip).  No HIP in here.  On top of gx_group.hpp (the keys, the per-slot words) and gx_bucket.hpp (bucket_of, the one-word
// table, the digit plan).
//
// The reference's caller asks for a series per captured text right behind the extraction (README.md:26,63-79, with a timestamp field):
//     r = gorp.extract(line);
//     if (r != null) {
//         long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
//         perVerb.computeIfAbsent(r.asMap().get("verb"), v -> new TreeMap<Long, Stats>())
//                .computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
//     }
// That is GROUP BY verb, floor((ts - origin) / width).  A PART is gx_group_lines' (extraction, key group, optional value group); beside
// it stands the part's NUMBER group (-1: its lines have a key and no number), parsed under its gx_number_format.  A line counts, is
// keyed or adds to `unset` exactly as in gx_group_lines.  A keyed line is CELLED when its part has a number group, that group names a
// value, the value parses and bucket_of gives a bucket; else it is number_unset (no number group, or the capture names nothing),
// not_numbers (the value does not parse) or out_of_range (bucket_of's rule): keyed == celled + number_unset + not_numbers +
// out_of_range.  Two celled lines are in the same CELL when they hold the same key and the same bucket number.  Cells leave ordered by
// (key number, bucket number): a series per key, in time order.  The distinct bucket numbers that hold a cell leave ascending, as an
// axis, and a cell names its bucket by its index into that axis.
//
// (key slot, bucket word) is 96 bits, and the tables rest on "a slot claimed by ONE 64-bit compare-and-swap is complete the moment it
// is visible".  So the buckets go through a one-word table of their own first (bucket_find_or_insert as it is), which gives a celled
// line a bucket slot below 2^31, and the cells live in a second one-word table keyed by
//     cell_word(kslot, bslot) = (kslot << 32 | bslot) + 1        never 0, never wraps: both indices are below 2^31
// The word is the whole key, so bucket_find_or_insert serves again, hashed by bucket_hash; the per-slot words are GROUP_W_* / GROUP_S_*.
// Both tables have group_slots(max_cells) slots: distinct buckets never exceed distinct cells.  Every merge is an unsigned integer add
// or maximum: every delivered bit is the same on every run.
//
// Not in scope: empty cells filled in, calendar widths (months, local days), quantiles per cell, ranking cells, lines per bucket across
// keys (that is gx_bucket_lines), more than one text key (compose with gx_group_pairs later).
#pragma once
#include <cstdint>

#include "gx_bucket.hpp"
#include "gx_group.hpp"

namespace gx {

constexpr uint64_t SERIES_MAX_CELLS = GROUP_MAX_KEYS;   // max_cells <= 2^30: group_slots gives at most 2^31 slots, slot numbers < 2^31
constexpr int32_t SERIES_NO_NUMBER = -1;                // SeriesHead::number of a part whose lines have a key and no number

GX_WHERE_HD uint64_t cell_word(uint32_t kslot, uint32_t bslot) { return ((static_cast<uint64_t>(kslot) << 32) | bslot) + 1u; }   // (kslot, bslot < 2^31)
GX_WHERE_HD uint32_t cell_kslot(uint64_t word) { return static_cast<uint32_t>((word - 1u) >> 32); }
GX_WHERE_HD uint32_t cell_bslot(uint64_t word) { return static_cast<uint32_t>(word - 1u); }

// The cells' sort word: ordered by (key number, rank of the bucket on the axis).  key_number < n_keys <= 2^30, bucket_rank < n_buckets
// <= 2^30: below 2^60.
GX_WHERE_HD uint64_t sort_word(uint64_t key_number, uint64_t bucket_rank, uint64_t n_buckets) { return key_number * n_buckets + bucket_rank; }
// The digits of the cells' sort: those of the largest sort word there can be, n_keys * n_buckets - 1, against 0.
GX_WHERE_HD uint32_t series_digits(uint64_t n_keys, uint64_t n_buckets) {
    const uint64_t words = n_keys * n_buckets;
    return words ? bucket_digits(0, words - 1u) : 0u;
}

// What the series adds to GroupHead, copied to LDS behind it: per entry of GroupHead::ext[] the number group and its packed format.
struct SeriesHead {
    int64_t origin;
    uint64_t width;                    // >= 1
    uint32_t flags;                    // GROUP_WEAK_HASH, BUCKET_ALL_DIGITS
    uint32_t formats;                  // != 0: some nfmt[] is not LONG
    uint32_t spare[2];
    int32_t number[GROUP_MAX_PARTS];   // SERIES_NO_NUMBER: none
    uint8_t nfmt[GROUP_MAX_PARTS];     // number[e]'s packed number format, 0 = LONG
};
static_assert(sizeof(SeriesHead) % 16 == 0, "the head is copied in 16-byte words");

// What the build pass leaves for the host, read in the ONE wait with the group totals, the buckets and the cells (status bit 2: a table
// is full).  min_inv is the maximum of ~word over the bucket words, max_word the maximum of word; both 0 without a cell.
struct SeriesDev {
    uint64_t celled, number_unset, not_numbers, out_of_range, status, min_inv, max_word, spare;
};
static_assert(sizeof(SeriesDev) == 64, "the host reads it from device memory as it is");

}  // namespace gx
