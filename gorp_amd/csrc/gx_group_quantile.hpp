// gx_group_quantile.hpp -- the rule of gx_group_quantiles, once: plain C++ for the host (g++ alone: tests/cpp/group_quantile_test.cpp)
// and for the kernels (gx_group_quantile.hip).  No HIP in here.  On top of gx_group.hpp (the keys, their numbers, a key's stats) and
// gx_quantile.hpp (quant_rank, QuantAsk, QuantOut; the class of a value and its order-preserving key are gx_top.hpp's).
//
// The reference's caller asks for percentiles of a captured number per captured text right behind the extraction (README.md:26,63-79):
//     byPath.computeIfAbsent(path, p -> new ArrayList<>()).add(Long.parseLong(timeTakenInMsec)); ... sorted(list)[ceil(q * size) - 1]
// A CANDIDATE is a line that has a key (gx_group_lines' rule) and whose value is a number (gx_top_lines' rule): the lines counted in
// key_stats[j].numbers.  Every candidate is a PAIR (value key, key number); the pairs are sorted by (key number, value key, input line)
// with a stable LSD radix sort of 6-bit digits, so that key j's population is one contiguous ascending run of the sorted pairs.  A
// quantile is then an index into the run, and `below` / `equal` are a lower and an upper bound inside it.
//
// THE DIGIT PLAN.  The value key's digits go first, least significant first, then the key number's.  A digit in which no two
// candidates differ cannot change the order and is not sorted: of the value key those are the digits where the OR and the AND of all
// candidates' value keys agree (bit b differs between two candidates exactly when it is set in OR ^ AND); of the key number the digits
// at and above bits(n_keys - 1).  Latency-like values differ in two or three digits out of eleven.  Pass p reads buffer p & 1 and
// writes buffer (p & 1) ^ 1: after the plan the pairs lie in buffer n_passes & 1.
#pragma once
#include <cstdint>

#include "gx_quantile.hpp"

namespace gx {

constexpr uint32_t GQ_DIGIT_BITS = 6, GQ_BINS = 1u << GQ_DIGIT_BITS;
constexpr uint32_t GQ_VALUE_DIGITS = (64u + GQ_DIGIT_BITS - 1u) / GQ_DIGIT_BITS;   // 11: the last one holds four bits
constexpr uint32_t GQ_KEY_DIGITS = (32u + GQ_DIGIT_BITS - 1u) / GQ_DIGIT_BITS;     // 6 (n_keys <= 2^30 needs five)
constexpr uint32_t GQ_MAX_PASSES = GQ_VALUE_DIGITS + GQ_KEY_DIGITS;

// the bits of the largest key number: 0 for one key (and for none)
GX_WHERE_HD uint32_t gq_key_bits(uint64_t n_keys) {
    uint32_t bits = 0;
    while (bits < 32u && n_keys > (1ull << bits)) ++bits;
    return bits;
}

struct GqPass {
    uint8_t on_key;   // 0: a digit of the value key, 1: of the key number
    uint8_t shift;    // the digit is (word >> shift) & 63
};
struct GqPlan {
    uint32_t n_passes;
    GqPass pass[GQ_MAX_PASSES];
};
// where the sorted pairs lie behind the plan's passes
GX_WHERE_HD uint32_t gq_result_buffer(const GqPlan& p) { return p.n_passes & 1u; }

// differ: OR ^ AND of the candidates' value keys (0 for fewer than two candidates); all_values: sort every value digit regardless
// (the measurement's other arm).  n_keys: the keys of the batch.
GX_WHERE_HD GqPlan gq_plan(uint64_t differ, uint64_t n_keys, bool all_values) {
    GqPlan p{};
    for (uint32_t d = 0; d < GQ_VALUE_DIGITS; ++d) {
        const uint32_t shift = d * GQ_DIGIT_BITS;
        if (all_values || ((differ >> shift) & (GQ_BINS - 1u)) != 0u) p.pass[p.n_passes++] = GqPass{0, static_cast<uint8_t>(shift)};
    }
    const uint32_t bits = gq_key_bits(n_keys);
    for (uint32_t shift = 0; shift < bits; shift += GQ_DIGIT_BITS) p.pass[p.n_passes++] = GqPass{1, static_cast<uint8_t>(shift)};
    return p;
}
GX_WHERE_HD uint32_t gq_digit(uint64_t word, uint32_t shift) { return static_cast<uint32_t>(word >> shift) & (GQ_BINS - 1u); }

// first index in [lo, hi) whose entry is >= x (lower) / > x (upper); hi if none.  a[] ascending in [lo, hi).
template <typename AP, typename T>
GX_WHERE_HD uint64_t gq_lower_bound(AP a, uint64_t lo, uint64_t hi, T x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] >= x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
template <typename AP, typename T>
GX_WHERE_HD uint64_t gq_upper_bound(AP a, uint64_t lo, uint64_t hi, T x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] > x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// Row (j, q) from the sorted pairs: knum[0, m) ascending, vkey[] ascending inside every key's run.  A key without numbers: zeros.
template <typename KP, typename VP>
GX_WHERE_HD QuantOut gq_pick(KP knum, VP vkey, uint64_t m, uint32_t j, uint32_t num, uint32_t den) {
    const uint64_t start = gq_lower_bound(knum, 0, m, j), end = gq_upper_bound(knum, start, m, j);
    const uint64_t rank = quant_rank(num, den, end - start);
    if (rank == 0u) return QuantOut{0, 0u, 0u, 0u};
    const uint64_t key = vkey[start + rank - 1u];   // (rank <= end - start)
    const uint64_t lo = gq_lower_bound(vkey, start, end, key), hi = gq_upper_bound(vkey, lo, end, key);
    return QuantOut{top_value(key, false), rank, lo - start, hi - lo};
}

// What lies at the head of the passes' device workspace; the host reads it in the wait in which it reads gx_group_lines' totals.
struct GqDev {
    uint32_t counts[TOP_COUNTS];   // the keys pass's class counts, over lines with and without a key
    uint64_t value_or, value_and;  // over the candidates' value keys; 0 and ~0 without a candidate
    uint64_t candidates;
    uint64_t spare;
};
static_assert(sizeof(GqDev) == 48, "the host reads it from device memory as it is");

}  // namespace gx
