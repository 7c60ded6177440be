// gx_quantile.hpp -- the rule of gx_capture_quantiles, once: plain C++ for the host (g++ alone: tests/cpp/quantile_test.cpp) and for the
// kernels (gx_quantile.hip).  No HIP in here.  On top of gx_top.hpp: the class of a line, the key and the radix select are gx_top_lines'.
//
// The reference's caller asks for percentiles of a number its lines captured right behind the extraction (README.md:26,63-79: the
// results' timeTakenInMsec).  The lines that count, and the class of each one's value, are gx_top_lines' (gx_top.hpp); the numbers are
// the population.  A quantile is num / den, and its rank is nearest-rank in integers alone: ceil(num * numbers / den), at least 1 --
// sorted(values)[rank - 1].  No floating point anywhere.
//
// The select runs on top_key(v, false): the rank-th smallest number is the (numbers - rank + 1)-th largest key, so a quantile's state
// is TopSelect's {prefix, remaining, above} plus `equal`, the count of the bin picked last: after digit 0 the numbers equal to the
// value.  Before digit d the quantiles whose prefixes agree above d form a GROUP and share one histogram; at digit 7 there is one group,
// and there are never more than QUANT_MAX.
#pragma once
#include <cstdint>

#include "gx_top.hpp"

namespace gx {

constexpr uint32_t QUANT_MAX = 16;   // (GX_QUANTILE_MAX: a sweep keeps a 256-bin histogram per group in LDS, 16 KiB)

// nearest rank: 1 <= rank <= numbers for numbers > 0 (0 for none).  num <= den, den >= 1, numbers < 2^32: the product cannot overflow.
GX_WHERE_HD uint64_t quant_rank(uint32_t num, uint32_t den, uint64_t numbers) {
    if (numbers == 0u) return 0u;
    const uint64_t p = static_cast<uint64_t>(num) * numbers;
    const uint64_t r = p / den + (p % den != 0u ? 1u : 0u);
    return r == 0u ? 1u : r;
}

struct QuantAsk {   // (gx_quantile as the device reads it)
    uint32_t num, den;
};

// A quantile's select as it stands between two digits.  rank == 0: no numbers, nothing to find, and no step changes anything.
struct QuantSelect {
    uint64_t prefix;      // the digits found so far, in place; after digit 0: the key of the value
    uint64_t rank;        // the rank asked for, 1 .. numbers
    uint32_t remaining;   // the key wanted is the remaining-th largest under the prefix
    uint32_t above;       // keys above everything under the prefix; after digit 0: the numbers above the value
    uint32_t equal;       // the count of the bin picked last; after digit 0: the numbers equal to the value
    uint32_t pad;
};
static_assert(sizeof(QuantSelect) == 32, "two of them per quantile lie in the device head");

struct QuantOut {   // (gx_quantile_out)
    int64_t value;
    uint64_t rank, below, equal;
};
static_assert(sizeof(QuantOut) == 32, "the host reads the rows from device memory as they are");

GX_WHERE_HD void quant_begin(QuantSelect& s, uint32_t num, uint32_t den, uint64_t numbers) {
    s.prefix = 0;
    s.rank = quant_rank(num, den, numbers);
    s.remaining = s.rank ? static_cast<uint32_t>(numbers - s.rank + 1u) : 0u;
    s.above = 0;
    s.equal = 0;
    s.pad = 0;
}

// The pick in a form that every bin can ask for itself: with S(b) = the sum of hist[b .. 255] (S(256) = 0), bin b is picked when
// S(b) >= remaining > S(b + 1).  For 1 <= remaining <= S(0) exactly one bin is, and it is top_pick's (tests/cpp/quantile_test.cpp).
GX_WHERE_HD bool quant_picked(uint64_t s_b, uint64_t s_b1, uint64_t remaining) { return s_b >= remaining && remaining > s_b1; }
GX_WHERE_HD TopPick quant_pick_of(uint32_t b, uint64_t s_b1, uint64_t remaining) {
    return TopPick{b, static_cast<uint32_t>(s_b1), static_cast<uint32_t>(remaining - s_b1)};
}

// digit d's step: p is the pick in the histogram of the quantile's group, bin_count that bin's count
GX_WHERE_HD void quant_step(QuantSelect& s, const TopPick& p, uint32_t bin_count, uint32_t d) {
    if (s.rank == 0u) return;
    s.prefix |= static_cast<uint64_t>(p.bin) << (8u * d);
    s.above += p.above;
    s.remaining = p.remaining;
    s.equal = bin_count;
}
// behind digit 0
GX_WHERE_HD QuantOut quant_out(const QuantSelect& s, uint64_t numbers) {
    if (s.rank == 0u) return QuantOut{0, 0u, 0u, 0u};
    return QuantOut{top_value(s.prefix, false), s.rank, numbers - s.above - s.equal, s.equal};
}

// The groups before digit d.  A quantile's representative is the lowest-numbered quantile whose prefix agrees with its own above d;
// the groups are numbered densely in the order of their representatives.
template <typename SP>
GX_WHERE_HD uint32_t quant_rep(SP s, uint32_t i, uint32_t d) {
    uint32_t j = 0;
    while (j < i && !top_in_prefix(s[j].prefix, s[i].prefix, d)) ++j;
    return j;
}
// rep[0 .. n_q): quant_rep of every quantile.  The group of quantile i, and the number of groups:
template <typename RP>
GX_WHERE_HD uint32_t quant_group_of(RP rep, uint32_t i) {
    uint32_t g = 0;
    for (uint32_t j = 0; j < rep[i]; ++j) g += rep[j] == j ? 1u : 0u;
    return g;
}
template <typename RP>
GX_WHERE_HD uint32_t quant_group_count(RP rep, uint32_t n_q) {
    uint32_t g = 0;
    for (uint32_t j = 0; j < n_q; ++j) g += rep[j] == j ? 1u : 0u;
    return g;
}
struct QuantGroups {
    uint32_t n_groups;
    uint8_t rep[QUANT_MAX];        // quantile -> its representative
    uint8_t group_of[QUANT_MAX];   // quantile -> its group, 0 .. n_groups - 1
    uint8_t head[QUANT_MAX];       // group -> its representative
};
template <typename SP>
GX_WHERE_HD void quant_groups(SP s, uint32_t n_q, uint32_t d, QuantGroups& g) {
    for (uint32_t i = 0; i < n_q; ++i) g.rep[i] = static_cast<uint8_t>(quant_rep(s, i, d));
    g.n_groups = quant_group_count(g.rep, n_q);
    for (uint32_t i = 0; i < n_q; ++i) {
        g.group_of[i] = static_cast<uint8_t>(quant_group_of(g.rep, i));
        if (g.rep[i] == i) g.head[g.group_of[i]] = static_cast<uint8_t>(i);
    }
}

// What lies at the head of the passes' device workspace.  The host reads the counts and the rows.  The select's state is kept twice:
// digit d's passes read sel[d & 1] and its pick writes sel[(d & 1) ^ 1], so that a pick's workgroups, one per quantile, can each work
// out the digit's grouping from every quantile's state while the others write theirs.
struct QuantDev {
    uint32_t counts[TOP_COUNTS];
    QuantOut out[QUANT_MAX];
    QuantSelect sel[2][QUANT_MAX];
};
static_assert(sizeof(QuantDev) == 16 + 32 * QUANT_MAX + 64 * QUANT_MAX, "counts, rows, state");

// The quantiles as the passes read them, built by the host behind the parts (TopHead) in the image.
struct QuantHead {
    uint32_t n_q, pad[3];
    QuantAsk ask[QUANT_MAX];
};
static_assert(sizeof(QuantHead) % 16 == 0, "the term image behind it is read in 16-byte words");

}  // namespace gx
