// gx_lookup.hpp -- the rule of gx_lookup_lines, once: plain C++ for the host (g++ alone: tests/cpp/lookup_test.cpp) and for the kernels
// (gx_lookup.hip).  No HIP in here.
//
// The reference's caller looks what a line captured up in a set or a map of its own right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null && wanted.contains(r.asMap().get("user"))) ...     meta = byHost.get(r.asMap().get("host"));
// A DICTIONARY is m texts the caller supplies as a CSR (units, m + 1 offsets) -- the form gx_group_lines leaves its keys in.  Two entries
// with the same units are duplicates and the LOWEST entry number stands for them all: index.putIfAbsent(entry[j], j) for ascending j.
// The entries live in gx_group.hpp's table -- the same hash, the same tag, group_slots(m) slots, so at most half of them are ever full --
// with an ENTRY number where gx_group_lines keeps a line number:
//     word = tag << 32 | (entry + 1), 0 = empty
// `entry` is SOME entry that holds the text (whichever duplicate claimed the slot: timing); beside the word the slot keeps the LOWEST
// entry with its text in group_first_word's complement form, merged by an unsigned maximum, and everything delivered comes from there.
// A line's key is looked up FIND-ONLY: the table is complete and nobody writes it while lines are probed, so a probe is plain loads, ends
// at an equal tag with equal units (a hit) or at the first empty slot (a miss), and visits every slot at most once.  Units are compared
// only behind an equal tag and an equal length, and nothing outside [value, value + length) of the key or the entry is read.
#pragma once
#include <cstdint>

#include "gx_group.hpp"

namespace gx {

constexpr uint64_t LOOKUP_MAX_ENTRIES = 1ull << 30;
constexpr uint32_t LOOKUP_NONE = 0xFFFFFFFFu;   // GX_LOOKUP_NONE: the line does not count, or its key pair names no value
constexpr uint32_t LOOKUP_MISS = 0xFFFFFFFEu;   // GX_LOOKUP_MISS: the line's key is set and is no entry (slots are below 2^31: never one)
enum : uint32_t { LOOKUP_KEEP_NOTHING = 0, LOOKUP_KEEP_HITS = 1, LOOKUP_KEEP_OTHERS = 2, LOOKUP_KEEPS };   // GX_LOOKUP_KEEP_* of include/gorp_hip.h
// what a line is to a dictionary: it does not count, or it counts and is exactly one of unset, hit, miss
enum : uint32_t { LOOKUP_SKIPPED = 0, LOOKUP_UNSET, LOOKUP_HIT, LOOKUP_IS_MISS };

GX_WHERE_HD uint32_t lookup_class(bool counts, bool key_set, uint32_t slot) {
    return !counts ? LOOKUP_SKIPPED : !key_set ? LOOKUP_UNSET : slot != LOOKUP_MISS ? LOOKUP_HIT : LOOKUP_IS_MISS;
}
// keep: hits are wanted.contains(v); others are !blocked.contains(v), v == null included; a line that does not count is never kept
GX_WHERE_HD bool lookup_keeps(uint32_t keep, uint32_t cls) {
    return keep == LOOKUP_KEEP_HITS ? cls == LOOKUP_HIT : keep == LOOKUP_KEEP_OTHERS ? (cls == LOOKUP_UNSET || cls == LOOKUP_IS_MISS) : false;
}

// the slot word of an entry (entry < 2^30)
GX_WHERE_HD uint64_t lookup_word(uint32_t tag, uint32_t entry) { return group_word(tag, entry); }
GX_WHERE_HD uint32_t lookup_word_entry(uint64_t word) { return group_word_line(word); }
// the lowest entry with a slot's text: the maximum of the complement is the minimum of the entry; 0: none
GX_WHERE_HD uint64_t lookup_low_word(uint32_t entry) { return group_first_word(entry); }
GX_WHERE_HD uint32_t lookup_low_entry(uint64_t word) { return group_first_line(word); }

// Find-only probe of the value v[0, vn).  Returns the slot that holds an entry with these units, or LOOKUP_MISS.
//   table.load(slot)          the slot's word
//   same(rep_entry, v, vn)    is entry rep_entry's text the value v[0, vn)?  (reads rep_entry's units from the dictionary)
// The table has group_slots(m) slots for m entries, so an empty slot ends every miss; the loop is bounded by the table besides.
template <typename Table, typename VP, typename Same>
GX_WHERE_HD uint32_t lookup_find(const Table& table, uint32_t n_slots, uint64_t hash, VP v, uint32_t vn, Same&& same) {
    const uint32_t tag = group_tag(hash);
    uint32_t slot = group_first_slot(hash, n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        const uint64_t cur = table.load(slot);
        if (cur == 0) return LOOKUP_MISS;
        if (group_tag(cur) == tag && same(lookup_word_entry(cur), v, vn)) return slot;
        slot = (slot + 1u) & (n_slots - 1u);
    }
    return LOOKUP_MISS;
}

}  // namespace gx
