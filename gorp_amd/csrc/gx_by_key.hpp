// gx_by_key.hpp -- the rule of gx_lines_by_key, once: plain C++ for the host (g++ alone: tests/cpp/by_key_test.cpp) and for the kernels
// (gx_by_key.hip).  No HIP in here.  On top of gx_group.hpp (the keys and their numbers) and gx_group_quantile.hpp (gq_key_bits,
// gq_digit, gq_lower_bound: the key number's digits and a key's run in the sorted key numbers).
//
// The reference's caller collects every key's lines right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) byRequest.computeIfAbsent(r.asMap().get("requestId"), k -> new ArrayList<>()).add(line);
// A key is KEPT when max(min_lines, 1) <= its lines and (max_lines == 0 or its lines <= max_lines); a line is kept when it has a key and
// the key is kept.  The kept lines are ENTRIES (key number, line number), written densely in line order and sorted by key number with a
// stable LSD radix sort of 6-bit digits: the order of the result is (key number, input line).  Key j's lines are then the run
// [lower_bound(j), lower_bound(j + 1)) of the sorted key numbers; a key that is not kept is an empty run.
//
// THE DIGIT PLAN.  ceil(bits(n_keys - 1) / 6) passes over the key number, least significant digit first: none for one key, five for 2^30
// keys, and five whatever n_keys is with BY_KEY_ALL_DIGITS (the digits above the largest key number are all zero: the passes move
// nothing out of order).  Pass p reads buffer p & 1 and writes buffer (p & 1) ^ 1: after the plan the entries lie in buffer n_passes & 1.
#pragma once
#include <cstdint>

#include "gx_group_quantile.hpp"

namespace gx {

constexpr uint32_t BY_KEY_ALL_DIGITS = 2u;    // GX_BY_KEY_ALL_DIGITS of include/gorp_hip.h
constexpr uint32_t BY_KEY_MAX_PASSES = 5;     // n_keys <= 2^30

GX_WHERE_HD bool by_key_kept(uint64_t lines, uint64_t min_lines, uint64_t max_lines) {
    return lines >= (min_lines ? min_lines : 1u) && (max_lines == 0u || lines <= max_lines);
}

GX_WHERE_HD uint32_t by_key_passes(uint64_t n_keys, bool all_digits) {
    return all_digits ? BY_KEY_MAX_PASSES : (gq_key_bits(n_keys) + GQ_DIGIT_BITS - 1u) / GQ_DIGIT_BITS;
}
GX_WHERE_HD uint32_t by_key_shift(uint32_t pass) { return pass * GQ_DIGIT_BITS; }
// where the sorted entries lie behind the plan's passes
GX_WHERE_HD uint32_t by_key_result_buffer(uint32_t n_passes) { return n_passes & 1u; }

// the first of key j's entries in knum[0, m) ascending: j's lines are [by_key_begin(j), by_key_begin(j + 1)); j = n_keys gives m
template <typename KP>
GX_WHERE_HD uint64_t by_key_begin(KP knum, uint64_t m, uint64_t j) {
    return gq_lower_bound(knum, 0, m, j);
}

// What the kept pass leaves at the head of the passes' device workspace; the host reads it in the wait in which it reads
// gx_group_lines' totals.
struct ByKeyDev {
    uint64_t lines_out, units_out, keys_kept, spare;
};
static_assert(sizeof(ByKeyDev) == 32, "the host reads it from device memory as it is");

}  // namespace gx
