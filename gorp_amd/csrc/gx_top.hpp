// gx_top.hpp -- the rule of gx_top_lines, once: plain C++ for the host (g++ alone: tests/cpp/top_test.cpp) and for the kernels
// (gx_top.hip).  No HIP in here.
//
// The reference's caller ranks lines by a number they captured right behind the extraction (README.md:26,63-79):
//     results.add(gorp.extract(line)) ...; sorted(results, by timeTakenInMsec).take(N)
// A PART names one extraction and the group whose value is the line's number; all parts share one number space.  A line counts when
// its outcome is an extraction that has a part and every term of that extraction holds (gx_where.hpp); its value is classed as
// gx_capture_stats classes one (where_pair_set, where_parse_int64): unset, no number, or a number.  The numbers are the candidates.
// The result is the n_top = min(N, numbers) candidates ordered by (value descending, input line ascending) -- or value ascending with
// `smallest` -- so ties at the cut go to the earliest lines.
//
// Both directions are "the n_top largest KEYS, ties to the lower line": top_key maps int64 to uint64 and keeps the order (it flips the
// sign bit), and for `smallest` takes the complement of that (never a negation: INT64_MIN has nothing to overflow).  The cut is found
// by an exact radix select over the key's eight 8-bit digits, most significant first: per digit a histogram of the keys whose higher
// digits equal the prefix found so far, and top_pick, which names the bin that holds the remaining-th largest of them.  After eight
// digits the prefix is the threshold key T, `above` counts the keys above T, and `remaining` = n_top - above of the keys equal to T
// are still to be taken: the earliest ones.
#pragma once
#include <cstdint>

#include "gx_where.hpp"

namespace gx {

constexpr uint32_t TOP_MAX_PARTS = 64;
constexpr uint32_t TOP_MAX_LINES = 4096;   // (GX_TOP_MAX_LINES: the order pass keeps that many keys in LDS, 32 KiB, and compares each with each)
constexpr uint32_t TOP_DIGITS = 8, TOP_BINS = 256;

GX_WHERE_HD uint64_t top_key(int64_t v, bool smallest) {
    const uint64_t k = static_cast<uint64_t>(v) ^ 0x8000000000000000ull;
    return smallest ? ~k : k;
}
GX_WHERE_HD int64_t top_value(uint64_t key, bool smallest) {
    const uint64_t k = smallest ? ~key : key;
    return static_cast<int64_t>(k ^ 0x8000000000000000ull);
}
// digit d of a key: d = 7 is the most significant
GX_WHERE_HD uint32_t top_digit(uint64_t key, uint32_t d) { return static_cast<uint32_t>(key >> (8u * d)) & 0xFFu; }
// do the key's digits above d equal the prefix's?  (the digits from d down are not looked at; above digit 7 there is nothing)
GX_WHERE_HD bool top_in_prefix(uint64_t key, uint64_t prefix, uint32_t d) {
    return d >= TOP_DIGITS - 1u || (key >> (8u * (d + 1u))) == (prefix >> (8u * (d + 1u)));
}

// The bin that holds the remaining-th largest key of a histogram (1 <= remaining <= the histogram's total): the highest bin b for
// which the keys in the bins above b are fewer than `remaining`.  above: the keys in the bins above it; remaining: what is still to be
// taken from the bin itself, 1 .. hist[bin].  Nothing outside hist[0, 256) is read.
struct TopPick {
    uint32_t bin, above, remaining;
};
template <typename HP>
GX_WHERE_HD TopPick top_pick(HP hist, uint32_t remaining) {
    uint64_t above = 0;
    uint32_t b = TOP_BINS - 1u;
    for (; b > 0u; --b) {
        const uint64_t h = hist[b];
        if (above + h >= remaining) break;
        above += h;
    }
    return TopPick{b, static_cast<uint32_t>(above), static_cast<uint32_t>(remaining - above)};
}

// The select as it stands between two digits.  n_top == 0: nothing to find, and no step changes anything.
struct TopSelect {
    uint64_t prefix;      // the digits found so far, in place; after digit 0: the threshold key T
    uint32_t remaining;   // keys still to be taken among those under the prefix; after digit 0: the ties that are taken
    uint32_t above;       // keys above everything under the prefix; after digit 0: the keys above T
    uint32_t n_top;       // min(N, numbers)
    uint32_t pad;
};
static_assert(sizeof(TopSelect) == 24, "the host reads it from device memory as it is");

GX_WHERE_HD void top_begin(TopSelect& s, uint32_t n_wanted, uint64_t numbers) {
    s.prefix = 0;
    s.n_top = numbers < n_wanted ? static_cast<uint32_t>(numbers) : n_wanted;
    s.remaining = s.n_top;
    s.above = 0;
    s.pad = 0;
}
// digit d's step: hist counts, by digit d, the keys for which top_in_prefix(key, s.prefix, d)
template <typename HP>
GX_WHERE_HD void top_step(TopSelect& s, HP hist, uint32_t d) {
    if (s.n_top == 0u) return;
    const TopPick p = top_pick(hist, s.remaining);
    s.prefix |= static_cast<uint64_t>(p.bin) << (8u * d);
    s.above += p.above;
    s.remaining = p.remaining;
}
// behind the last step: is a candidate with this key chosen?  eq_rank: the candidates with the same key on lines before it.
GX_WHERE_HD bool top_chosen(const TopSelect& s, uint64_t key, uint64_t eq_rank) {
    return s.n_top != 0u && (key > s.prefix || (key == s.prefix && eq_rank < s.remaining));
}

// The parts as the keys pass reads them, built by the host (gx_api.cpp: top_image) and copied to LDS by every workgroup: the
// extractions that have a part, ascending (searched with where_find), and each one's value group.
struct TopHead {
    uint32_t n_parts, smallest;
    uint32_t formats;                // != 0: some fmt[] is not LONG -- the host launches the keys pass's instantiation that reads them
    uint32_t pad;
    uint32_t ext[TOP_MAX_PARTS];
    uint16_t group[TOP_MAX_PARTS];
    uint8_t fmt[TOP_MAX_PARTS];      // group[e]'s packed number format (gx_number.hpp), 0 = LONG
};
static_assert(sizeof(TopHead) % 16 == 0, "the head is copied in 16-byte words");

// What lies at the head of the passes' device workspace, and what the host reads of it (the counts and the select): the summed class
// counts, the select's state, and the current digit's summed histogram.
enum : uint32_t { TOP_C_NUMBERS = 0, TOP_C_UNSET, TOP_C_NOT_NUMBERS, TOP_C_STATUS, TOP_COUNTS };   // (status != 0: a line of 4 G code units)
struct TopDev {
    uint32_t counts[TOP_COUNTS];
    TopSelect sel;
    uint64_t spare;
    uint32_t hist[TOP_BINS];
};
static_assert(sizeof(TopDev) == 48 + 4 * TOP_BINS, "counts, select, histogram");

}  // namespace gx
