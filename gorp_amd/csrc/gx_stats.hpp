// gx_stats.hpp -- the rule of gx_capture_stats, once: plain C++ for the host (g++ alone: tests/cpp/stats_test.cpp) and for the
// kernel (gx_stats.hip).  No HIP in here.
//
// The reference's caller measures what a line captured right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) metrics.record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
// A MEASURE is one group of one extraction.  Every line of the extraction that counts (gx_where.hpp: every term of the extraction
// holds) falls into one of three classes: the group's offset pair names no value (where_pair_set) -- unset; where_parse_int64 rejects
// the value -- no number; or it is a number, which adds to the count, the minimum, the maximum, the exact sum and one histogram
// bucket.  The sum is kept as two partial sums that cannot overflow below 2^32 numbers, lo = sum (uint32_t)v and hi = sum (v >> 32),
// and joined in 128 bits at the very end (stats_sum128): integer addition is associative, so any order of merging gives the same bits.
#pragma once
#include <cstdint>

#include "gx_where.hpp"

namespace gx {

constexpr uint32_t STATS_MAX_MEASURES = 64;
constexpr uint32_t STATS_MAX_EDGES = 64;          // of one measure (StatsMeasure::n_edges is a byte)
constexpr uint32_t STATS_MAX_EDGES_TOTAL = 1024;  // of a call
constexpr int64_t STATS_INT64_MAX = 0x7FFFFFFFFFFFFFFFll, STATS_INT64_MIN = -STATS_INT64_MAX - 1;

// The bucket of v: the number of edges that are <= v (edges strictly ascending, n_edges <= 64).  Bucket 0 is v < edges[0], bucket
// n_edges is v >= edges[n_edges - 1].  A binary search of at most seven steps; nothing outside edges[0, n_edges) is read.
template <typename EP>
GX_WHERE_HD uint32_t stats_bucket(EP edges, uint32_t n_edges, int64_t v) {
    uint32_t lo = 0, hi = n_edges;
    for (int s = 0; s < 7; ++s) {
        if (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (edges[mid] <= v) lo = mid + 1;
            else hi = mid;
        }
    }
    return lo;
}

// (v >> 32 of a negative v, without leaning on what >> does to one: floor(v / 2^32))
GX_WHERE_HD int64_t stats_high(int64_t v) {
    const uint64_t u = static_cast<uint64_t>(v) >> 32;                       // the upper word, zero-extended
    return static_cast<int64_t>(u) - ((u & 0x80000000ull) ? (1ll << 32) : 0);   // ... sign-extended
}

// One measure's running summary.  lines == numbers + unset + not_numbers.
struct StatsAcc {
    uint64_t numbers = 0, unset = 0, not_numbers = 0;
    int64_t min = STATS_INT64_MAX, max = STATS_INT64_MIN;
    uint64_t lo = 0;   // sum of the numbers' low 32 bits
    int64_t hi = 0;    // sum of floor(v / 2^32)

    GX_WHERE_HD void add_number(int64_t v) {
        ++numbers;
        if (v < min) min = v;
        if (v > max) max = v;
        lo += static_cast<uint64_t>(v) & 0xFFFFFFFFull;
        hi += stats_high(v);
    }
    GX_WHERE_HD void add_unset() { ++unset; }
    GX_WHERE_HD void add_not_number() { ++not_numbers; }
    GX_WHERE_HD void merge(const StatsAcc& o) {
        numbers += o.numbers;
        unset += o.unset;
        not_numbers += o.not_numbers;
        if (o.min < min) min = o.min;
        if (o.max > max) max = o.max;
        lo += o.lo;
        hi += o.hi;
    }
    GX_WHERE_HD uint64_t lines() const { return numbers + unset + not_numbers; }
};

// hi * 2^32 + lo as a 128-bit two's-complement integer (sum_hi : sum_lo), in 64-bit pieces so that nothing wraps but the carry.
GX_WHERE_HD void stats_sum128(uint64_t lo, int64_t hi, uint64_t* sum_lo, int64_t* sum_hi) {
    const uint64_t h = static_cast<uint64_t>(hi);
    const uint64_t low = h << 32;                               // bits 0 .. 63 of hi * 2^32
    const int64_t high = stats_high(hi);                        // bits 64 .. 127: floor(hi / 2^32)
    const uint64_t s = low + lo;                                // (unsigned: the carry is what wraps)
    *sum_lo = s;
    *sum_hi = high + (s < low ? 1 : 0);
}

// Classes a value and adds it.  Returns the number's histogram bucket, or 0xFFFFFFFF when the line added no number.
template <typename VP, typename EP>
GX_WHERE_HD uint32_t stats_add(StatsAcc& a, bool pair_set, VP value, uint32_t units, EP edges, uint32_t n_edges) {
    int64_t v = 0;
    if (!pair_set) { a.add_unset(); return 0xFFFFFFFFu; }
    if (!where_parse_int64(value, units, &v)) { a.add_not_number(); return 0xFFFFFFFFu; }
    a.add_number(v);
    return stats_bucket(edges, n_edges, v);
}

// The measures as the kernel reads them, built by the host (gx_api.cpp: stats_image) and copied to LDS by every workgroup: the head,
// then the edges (int64, one measure's behind the other's).  The measures are ordered by extraction; ext[] holds the extractions that
// have measures, ascending, and extraction ext[e]'s measures are m[first[e] .. first[e + 1]) (WhereHead's scheme, searched with
// where_find).  hist_at: the measure's first bin among the call's bins, which lie in the caller's order.
struct StatsMeasure {
    uint16_t group;
    uint8_t n_edges;    // <= STATS_MAX_EDGES
    uint8_t fmt;        // the group's packed number format (gx_number.hpp), 0 = LONG
    uint16_t edge_at;   // first edge among the edges
    uint16_t hist_at;   // first of its n_edges + 1 bins
};
struct StatsHead {
    uint32_t n_measures, n_ext, n_edges, n_bins;
    uint32_t ext[STATS_MAX_MEASURES];
    uint8_t first[STATS_MAX_MEASURES + 16];   // n_ext + 1 entries
    StatsMeasure m[STATS_MAX_MEASURES];
};
static_assert(sizeof(StatsMeasure) == 8 && sizeof(StatsHead) % 16 == 0, "the head is copied in 16-byte words, the edges behind it are 8-byte aligned");

// A measure's eight 64-bit words in a workgroup's LDS, in its slab and in the summed result: three counts, a spare, min, max, lo, hi.
enum : uint32_t { STATS_W_NUMBERS = 0, STATS_W_UNSET, STATS_W_NOT_NUMBERS, STATS_W_SPARE, STATS_W_MIN, STATS_W_MAX, STATS_W_LO, STATS_W_HI, STATS_WORDS };

}  // namespace gx
