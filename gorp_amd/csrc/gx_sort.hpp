// gx_sort.hpp -- the rule of gx_sort_lines, once: plain C++ for the host (g++ alone: tests/cpp/sort_test.cpp) and for the kernels
// (gx_sort.hip).  No HIP in here.  On top of gx_top.hpp (which lines count, the class of a value, top_key / top_value),
// gx_bucket.hpp (bucket_digit: six-bit digit d of a 64-bit word) and gx_group_quantile.hpp (GQ_*: the digits' width and number,
// gq_lower_bound).
//
// The reference's caller puts two hosts' logs, or a log written by several threads, in time order right behind the extraction
// (README.md:26,63-79):
//     results.sort(Comparator.comparingLong(r -> Instant.parse(r.asMap().get("ts")).toEpochMilli()));
// Parts are gx_top_lines' parts.  A line is
//   STAMPED  when it counts by gx_top_lines' rule and its value is a number: its key is top_key(value, descending);
//   CARRIED  (with SORT_CARRY only) when it is not stamped and some earlier line of the batch is: it takes the key of the nearest
//            earlier stamped line -- a stack trace travels with the line above it;
//   REST     otherwise: without SORT_CARRY every line that is not stamped, with it the lines before the first stamped line.
// The stamped and carried lines are the ENTRIES, m of them; they leave ordered by (key ascending, input line ascending), which is
// value ascending, or value descending with SORT_DESCENDING, ties by input line in both directions.  A carried line has its header's
// key and a larger line number: a record leaves intact and in order.  With SORT_REST_LAST the rest lines follow in input order,
// else they are dropped.
//
// PLACES.  before[i] = the stamped lines before line i (before[n]: all of them), ckeys[] = the stamped lines' keys in line order:
// line i carries ckeys[before[i] - 1].  With carry the entries are exactly the lines from the first stamped line on: L = the lines
// before it (n without one), m = n - L, entry i sits at i - L.  Without carry m = before[n] and entry i sits at before[i].  Rest line
// i sits at m + i - before[i] in both cases (with carry before[i] is 0 there).
//
// THE DIGIT PLAN.  A stable LSD radix sort of the (key, line) pairs over six-bit digits, least significant first; digit d is
// bucket_digit(key, d), digit 10 holds four bits.  A digit in which no two entries differ cannot change the order and is not sorted:
// those are the digits where the OR and the AND of all entries' keys agree (gx_group_quantile.hpp gives the argument).  Fewer than
// two distinct keys: no pass at all.  SORT_ALL_DIGITS sorts all eleven (m > 0): the same result, only slower.  Pass p reads buffer
// p & 1 and writes buffer (p & 1) ^ 1: after the plan the pairs lie in buffer n_passes & 1.
#pragma once
#include <cstdint>

#include "gx_bucket.hpp"
#include "gx_group_quantile.hpp"

namespace gx {

constexpr uint32_t SORT_DESCENDING = 1u, SORT_CARRY = 2u, SORT_REST_LAST = 4u, SORT_ALL_DIGITS = 8u;   // GX_SORT_* of include/gorp_hip.h
constexpr uint32_t SORT_FLAGS = 15u;
constexpr uint64_t SORT_MAX_LINES = 1ull << 30;        // what the pair sort's kernels state (gx_bucket_sort_dev.hpp)
constexpr uint32_t SORT_MAX_PASSES = GQ_VALUE_DIGITS;  // 11
static_assert(GQ_DIGIT_BITS == BUCKET_DIGIT_BITS && SORT_MAX_PASSES == BUCKET_MAX_DIGITS, "one digit width for the plan and the sort's kernels");

enum : uint32_t { SORT_STAMPED = 0, SORT_CARRIED = 1, SORT_REST = 2 };   // gx_sort_out.out_class

// stamped: the line's value is a number (the keys pass's candidate flag); before: the stamped lines before it
GX_WHERE_HD uint32_t sort_class(bool stamped, uint64_t before, bool carry) {
    return stamped ? SORT_STAMPED : (carry && before > 0u) ? SORT_CARRIED : SORT_REST;
}
// the lines before the first stamped line (n without one): before[0 .. n] ascending, before[0] = 0
template <typename BP>
GX_WHERE_HD uint64_t sort_leading(BP before, uint64_t n) {
    return gq_lower_bound(before, 0, n + 1u, static_cast<uint64_t>(1)) - 1u;
}
GX_WHERE_HD uint64_t sort_entries(uint64_t n, uint64_t stamped, uint64_t leading, bool carry) { return carry ? n - leading : stamped; }
// an entry's key (cls SORT_STAMPED or SORT_CARRIED; a carried line has before > 0)
template <typename KP>
GX_WHERE_HD uint64_t sort_entry_key(KP ckeys, uint32_t cls, uint64_t before) {
    return ckeys[cls == SORT_STAMPED ? before : before - 1u];
}
GX_WHERE_HD uint64_t sort_entry_at(uint64_t i, uint64_t before, uint64_t leading, bool carry) { return carry ? i - leading : before; }
GX_WHERE_HD uint64_t sort_rest_at(uint64_t i, uint64_t before, uint64_t m) { return m + i - before; }

struct SortPlan {
    uint32_t n_passes;
    uint8_t digit[SORT_MAX_PASSES];   // pass p sorts by bucket_digit(key, digit[p])
};
// key_or, key_and: over the m entries' keys
GX_WHERE_HD SortPlan sort_plan(uint64_t key_or, uint64_t key_and, uint64_t m, bool all_digits) {
    SortPlan p{};
    if (m == 0u) return p;
    const uint64_t differ = m < 2u ? 0ull : key_or ^ key_and;
    for (uint32_t d = 0; d < SORT_MAX_PASSES; ++d)
        if (all_digits || bucket_digit(differ, d) != 0u) p.digit[p.n_passes++] = static_cast<uint8_t>(d);
    return p;
}
// where the sorted pairs lie behind the plan's passes
GX_WHERE_HD uint32_t sort_result_buffer(uint32_t n_passes) { return n_passes & 1u; }

// What the totals pass leaves at the head of the passes' device workspace; the host reads it in its one wait.
struct SortDev {
    uint32_t counts[TOP_COUNTS];       // the keys pass's class counts; [TOP_C_STATUS] != 0: a line of 4 G code units, or offsets that go backwards
    uint64_t key_or, key_and;          // over the entries' keys; 0 and ~0 without one
    uint64_t key_min, key_max;         // the first and the last entry's key in output order; ~0 and 0 without one
    uint64_t entries, carried, rest;   // m; the carried ones among them; the rest lines
    uint64_t units_out;                // the code units of the lines that leave
    uint64_t unordered;                // != 0: some entry's key is below the key of the entry before it in line order
    uint64_t leading;                  // the lines before the first stamped line
};
static_assert(sizeof(SortDev) == 16 + 10 * 8, "the host reads it from device memory as it is");

}  // namespace gx
