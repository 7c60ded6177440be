// gx_pairs.hpp -- the rule of gx_group_pairs, once: plain C++ for the host (g++ alone: tests/cpp/pairs_test.cpp) and for the kernels
// (gx_pairs.hip).  No HIP in here.  On top of gx_group.hpp: the keys, their slots, the slot word and find-or-insert are that header's.
//
// The reference's caller keys on TWO captured texts right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line);
//     if (r != null) seen.computeIfAbsent(r.asMap().get("verb"), v -> new HashSet<>()).add(r.asMap().get("path"));
//     if (r != null) byBoth.merge(List.of(r.asMap().get("verb"), r.asMap().get("path")), 1L, Long::sum);
// A part is gx_group_lines' part plus a SECOND group (-1: none).  A line counts, is keyed or adds to `unset` exactly as in
// gx_group_lines.  A keyed line is PAIRED when its part has a second group and that group's pair names a value (where_pair_set: an unset
// group, begin < 0 <= end, end < begin or an end beyond the line is never dereferenced); every other keyed line is UNPAIRED, so
// keyed == paired + unpaired.  The empty second is a value like any other.  Two paired lines hold the same PAIR when they have the same
// key -- the same key SLOT of gx_group_lines' table, which is finished before the pair pass starts -- and their seconds have the same
// number of units and the same units.  The seconds of different parts live in one space, as the keys do.  Pairs leave ordered by the
// first input line that holds them.
//
// The pairs live in a second hash table of gx_group.hpp's slot words: tag << 32 | (line + 1), 0 = empty, `line` SOME line that holds the
// pair (its representative).  A slot holds no copy of the pair: the representative's second is read from the batch and its key slot from
// slot_of[], both finished before the pass starts and written by nobody during it.  So gx_group.hpp's argument carries over verbatim: a
// slot that another lane has just claimed is complete the moment its word is visible -- no flag, no fence, no lane that waits for
// another lane.  Which line represents a slot depends on timing; nothing that is delivered does.  Every loop is bounded by the table:
// group_find_or_insert visits every slot at most once, then reports GROUP_NONE ("full").
//
// Not in scope: stats per pair, quantiles per pair, ranking pairs, more than two texts.
#pragma once
#include <cstdint>

#include "gx_group.hpp"

namespace gx {

constexpr uint64_t PAIRS_MAX_PAIRS = GROUP_MAX_KEYS;   // max_pairs <= 2^30: group_slots gives at most 2^31 slots
constexpr int32_t PAIRS_NO_SECOND = -1;                // PairsHead::second of a part whose lines have a key and no second

// The 64-bit hash of a pair: group_hash of the second's units (NOT cut: weak = false there) with the key slot mixed in by a multiply
// with an odd constant, then group_hash's finishing mix, so that the upper half (the tag) and the lower bits (the first slot) depend
// on both.  weak: GX_GROUP_WEAK_HASH's cut to the low 3 bits -- eight hashes in all, tag 0.
GX_WHERE_HD uint64_t pair_hash(uint64_t second_hash, uint32_t key_slot, bool weak) {
    uint64_t h = second_hash ^ ((static_cast<uint64_t>(key_slot) + 1u) * 0x9E3779B97F4A7C15ull);
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return weak ? (h & 7ull) : h;
}

// pair equality: the same key slot, the same number of units and the same units
template <typename AP, typename BP>
GX_WHERE_HD bool pair_same(uint32_t a_slot, AP a, uint32_t an, uint32_t b_slot, BP b, uint32_t bn) {
    return a_slot == b_slot && group_same_key(a, an, b, bn);
}

// Find-or-insert of the pair (key_slot, v[0, vn)) of line `line`: the pair's slot, or GROUP_NONE when every slot holds another pair.
//   table            group_find_or_insert's policy (load, claim) over the PAIR table's words
//   pair_of_line(r, &slot, &units)   line r's key slot and its second's units (r is paired: it is in the table); returns the units
template <typename Table, typename VP, typename PairOfLine>
GX_WHERE_HD uint32_t pair_find_or_insert(Table& table, uint32_t n_slots, uint32_t key_slot, uint32_t line, VP v, uint32_t vn, bool weak,
                                         PairOfLine&& pair_of_line) {
    const uint64_t hash = pair_hash(group_hash(v, vn, false), key_slot, weak);
    return group_find_or_insert(table, n_slots, hash, line, v, vn, [&](uint32_t rep, VP a, uint32_t an) {
        if (rep == line) return true;
        uint32_t b_slot = GROUP_NONE, bn = 0;
        const VP b = pair_of_line(rep, b_slot, bn);
        return pair_same(key_slot, a, an, b_slot, b, bn);
    });
}

// The pair table on the host: plain words, gx_group.hpp's policy.
typedef GroupHostTable PairsHostTable;

// The second groups as the kernels read them, built by the host (gx_api.cpp) and copied to LDS behind GroupHead: second[q] belongs to
// GroupHead::ext[q] / part[q].
struct PairsHead {
    int32_t second[GROUP_MAX_PARTS];   // PAIRS_NO_SECOND: none
    uint32_t pad[4];
};
static_assert(sizeof(PairsHead) % 16 == 0, "the head is copied in 16-byte words");

// A pair slot's words beside the table are GROUP_W_LINES and GROUP_W_FIRST in gx_group.hpp's forms.  What the passes leave for the host,
// read in the wait in which it reads gx_group_lines' totals (status bit 2: the pair table is full):
struct PairsDev {
    uint64_t paired, unpaired, status, spare[5];
};
static_assert(sizeof(PairsDev) == 64, "the host reads it from device memory as it is");

}  // namespace gx
