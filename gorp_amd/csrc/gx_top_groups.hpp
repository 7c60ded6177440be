// gx_top_groups.hpp -- the rule of gx_top_groups, once: plain C++ for the host (g++ alone: tests/cpp/top_groups_test.cpp) and for the
// kernels (gx_top_groups.hip).  No HIP in here.  On top of gx_group.hpp (the keys, their numbers, a key's words) and gx_top.hpp
// (top_pick, TopPick).
//
// The reference's caller asks which keys are the biggest right behind the extraction (README.md:26,63-79), on the map that
// gx_group_lines builds:
//     byPath.merge(r.asMap().get("path"), 1L, Long::sum); ... byPath.entrySet().stream().sorted(comparingByValue().reversed()).limit(10)
// Keys, parts, terms, which lines count, key equality, the one key space and the key numbers (order of first line) are
// gx_group_lines'.  Every key has a RANK VALUE, a signed 128-bit integer chosen by rank_by: its lines, its numbers, the exact sum of its
// numbers, their maximum or their minimum (the last three: only keys with a number are candidates).  The result is the n_top =
// min(n_wanted, candidates) candidates ordered by (rank value descending, key number ascending) -- ascending with `smallest` -- so
// ties at the cut go to the keys that appeared first: gx_top_lines' tie rule, one level up.
//
// Both directions are "the n_top largest KEYS, ties to the lower key number": tg_key maps the rank value to an unsigned 128-bit key
// (hi, lo) and keeps the order -- the sign bit flipped, and for `smallest` the complement of that, never a negation; top_key for two
// words.  The cut is an exact radix select over the key's sixteen 8-bit digits, most significant first, with top_pick per digit.
//
// THE DIGIT PLAN.  A digit in which no two candidates differ cannot decide anything: there the OR and the AND of the candidates' keys
// agree, the histogram would have one bin, and the prefix takes the digit from the OR.  Counts of ten million lines differ in three or
// four digits out of sixteen (gq_plan's argument, gx_group_quantile.hpp).
//
// No floating point anywhere.  Ranking by the MEAN is deliberately left out: comparing a/b with c/d exactly needs 192-bit products
// (a 128-bit sum times a 64-bit count) -- the next step, as a third key word.  Ranking by a per-key quantile is left out too.
#pragma once
#include <cstdint>

#include "gx_group.hpp"
#include "gx_top.hpp"

namespace gx {

constexpr uint32_t TG_MAX = 4096;        // GX_TOP_GROUPS_MAX: the cap on n_wanted, TOP_MAX_LINES'
constexpr uint32_t TG_SMALLEST = 2u;     // GX_TOP_GROUPS_SMALLEST; GROUP_WEAK_HASH (1u) shares the flags word
constexpr uint32_t TG_DIGITS = 16;
enum : uint32_t { TG_RANK_LINES = 0, TG_RANK_NUMBERS, TG_RANK_SUM, TG_RANK_MAX, TG_RANK_MIN, TG_RANK_KINDS };

struct TgKey {
    uint64_t hi, lo;
};
GX_WHERE_HD bool tg_above(const TgKey& a, const TgKey& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
GX_WHERE_HD bool tg_equal(const TgKey& a, const TgKey& b) { return a.hi == b.hi && a.lo == b.lo; }

// the rank value (hi : lo, two's complement) <-> the key
GX_WHERE_HD TgKey tg_key(int64_t hi, uint64_t lo, bool smallest) {
    const TgKey k{static_cast<uint64_t>(hi) ^ 0x8000000000000000ull, lo};
    return smallest ? TgKey{~k.hi, ~k.lo} : k;
}
GX_WHERE_HD void tg_value(const TgKey& key, bool smallest, int64_t* hi, uint64_t* lo) {
    const TgKey k = smallest ? TgKey{~key.hi, ~key.lo} : key;
    *hi = static_cast<int64_t>(k.hi ^ 0x8000000000000000ull);
    *lo = k.lo;
}

// Key j's rank value from its slot's words: head[GROUP_HEAD_WORDS], and stats[GROUP_STATS_WORDS], which is read only when has_values
// (without values the slots have no stats words, and only TG_RANK_LINES is legal).  Returns whether the key is a candidate.
template <typename HP, typename SP>
GX_WHERE_HD bool tg_rank_value(uint32_t rank_by, bool has_values, HP head, SP stats, int64_t* hi, uint64_t* lo) {
    *hi = 0;
    *lo = 0;
    if (rank_by == TG_RANK_LINES) { *lo = head[GROUP_W_LINES]; return true; }
    if (!has_values) return false;
    const uint64_t numbers = stats[GROUP_S_NUMBERS];
    if (rank_by == TG_RANK_NUMBERS) { *lo = numbers; return true; }
    if (numbers == 0u) return false;
    if (rank_by == TG_RANK_SUM) {
        stats_sum128(stats[GROUP_S_LO], static_cast<int64_t>(stats[GROUP_S_HI]), lo, hi);
        return true;
    }
    const int64_t v = rank_by == TG_RANK_MAX ? group_max_of(stats[GROUP_S_MAX]) : group_min_of(stats[GROUP_S_MIN]);
    *lo = static_cast<uint64_t>(v);
    *hi = v < 0 ? -1 : 0;
    return true;
}

// digit d of a key: d = 15 is the most significant
GX_WHERE_HD uint32_t tg_digit(const TgKey& k, uint32_t d) {
    return static_cast<uint32_t>(d >= 8u ? k.hi >> (8u * (d - 8u)) : k.lo >> (8u * d)) & 0xFFu;
}
// do the key's digits above d equal the prefix's?  (the digits from d down are not looked at; above digit 15 there is nothing)
GX_WHERE_HD bool tg_in_prefix(const TgKey& k, const TgKey& prefix, uint32_t d) {
    if (d >= 8u) return d >= TG_DIGITS - 1u || (k.hi >> (8u * (d - 7u))) == (prefix.hi >> (8u * (d - 7u)));
    return k.hi == prefix.hi && (d == 7u || (k.lo >> (8u * (d + 1u))) == (prefix.lo >> (8u * (d + 1u))));
}

// The plan: bit d set = digit d is selected on.  key_or / key_and: over the candidates' keys (0 and ~0 without a candidate: no digit).
GX_WHERE_HD uint32_t tg_plan(const TgKey& key_or, const TgKey& key_and) {
    const TgKey differ{key_or.hi & ~key_and.hi, key_or.lo & ~key_and.lo};
    uint32_t plan = 0;
    for (uint32_t d = 0; d < TG_DIGITS; ++d)
        if (tg_digit(differ, d) != 0u) plan |= 1u << d;
    return plan;
}

// The select as it stands between two digits.  n_top == 0: nothing to find, and no step changes anything.
struct TgSelect {
    TgKey prefix;         // the digits found so far, in place; after digit 0: the threshold key T
    uint32_t remaining;   // keys still to be taken among those under the prefix; after digit 0: the ties that are taken
    uint32_t above;       // keys above everything under the prefix; after digit 0: the keys above T
    uint32_t n_top;       // min(n_wanted, candidates)
    uint32_t plan;        // tg_plan
};
static_assert(sizeof(TgSelect) == 32, "the host reads it from device memory as it is");

GX_WHERE_HD void tg_begin(TgSelect& s, uint32_t n_wanted, uint64_t candidates, const TgKey& key_or, const TgKey& key_and) {
    s.prefix = TgKey{0, 0};
    s.n_top = candidates < n_wanted ? static_cast<uint32_t>(candidates) : n_wanted;
    s.remaining = s.n_top;
    s.above = 0;
    s.plan = candidates ? tg_plan(key_or, key_and) : 0u;
}
GX_WHERE_HD bool tg_planned(const TgSelect& s, uint32_t d) { return s.n_top != 0u && ((s.plan >> d) & 1u) != 0u; }
// digit d's step.  A planned digit: hist counts, by digit d, the candidates for which tg_in_prefix(key, s.prefix, d).  A skipped one:
// every candidate holds the OR's digit there; hist is not read.
template <typename HP>
GX_WHERE_HD void tg_step(TgSelect& s, HP hist, uint32_t d, const TgKey& key_or) {
    if (s.n_top == 0u) return;
    uint64_t digit = tg_digit(key_or, d);
    if (tg_planned(s, d)) {
        const TopPick p = top_pick(hist, s.remaining);
        digit = p.bin;
        s.above += p.above;
        s.remaining = p.remaining;
    }
    if (d >= 8u) s.prefix.hi |= digit << (8u * (d - 8u));
    else s.prefix.lo |= digit << (8u * d);
}
// behind the last step: is a candidate with this key chosen?  eq_rank: the candidates with the same key and a lower key number.
GX_WHERE_HD bool tg_chosen(const TgSelect& s, const TgKey& key, uint64_t eq_rank) {
    return s.n_top != 0u && (tg_above(key, s.prefix) || (tg_equal(key, s.prefix) && eq_rank < s.remaining));
}

// What lies at the head of the passes' device workspace; the host reads it (without the histogram) in its second wait.
struct TgDev {
    uint64_t candidates;
    TgKey key_or, key_and;   // over the candidates' keys; 0 and ~0 without a candidate
    TgSelect sel;
    uint64_t spare;
    uint32_t hist[TOP_BINS];
};
static_assert(sizeof(TgDev) == 80 + 4 * TOP_BINS, "candidates, OR, AND, select, histogram");

}  // namespace gx
