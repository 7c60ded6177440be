// gx_group.hpp -- the rule of gx_group_lines, once: plain C++ for the host (g++ alone: tests/cpp/group_test.cpp) and for the kernel
// (gx_group.hip).  No HIP in here.
//
// The reference's caller keys on what a line captured right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) byVerb.merge(r.asMap().get("verb"), 1L, Long::sum);
// A PART names, for the lines of one extraction, the group whose value is the line's KEY and optionally a group whose value is
// measured per key as gx_capture_stats measures one (gx_stats.hpp).  Two values are the same key when they have the same number of
// code units and the same units.  The keys live in a hash table of 64-bit slot words built on the device:
//     word = tag << 32 | (line + 1), 0 = empty
// where `line` is SOME line that holds the key (its representative) and tag the upper half of the value's hash.  A slot holds no copy
// of the key: the units are read from the batch, which nobody writes during the call, so a slot that another lane has just claimed is
// complete the moment its word is visible -- no flag, no fence, no lane that waits for another lane.  Which line represents a slot
// depends on timing; nothing that is delivered does.  Every loop is bounded: a slot goes from empty to full once and never back, so a
// failed claim hands back the word that beat it and the slot is not read again; probing visits every slot at most once, then reports
// "full".  Units are compared only behind an equal tag and an equal length, and nothing outside [value, value + length) of either line
// is read.
#pragma once
#include <cstdint>

#include "gx_stats.hpp"
#include "gx_where.hpp"

namespace gx {

constexpr uint32_t GROUP_MAX_PARTS = 64;
constexpr uint64_t GROUP_MAX_KEYS = 1ull << 30;
constexpr uint32_t GROUP_WEAK_HASH = 1u;          // GX_GROUP_WEAK_HASH of include/gorp_hip.h
constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;      // slot_of / line_key of a line that has no key; find-or-insert's "full"
constexpr uint32_t GROUP_NO_VALUE = 0xFFFFu;      // GroupPart::value_group of a part that only counts
// a workgroup's LDS table of the slots it adds to (gx_group.hip): entries, and how many of them are ever claimed -- half, so that
// probing meets a free entry soon
constexpr uint32_t GROUP_LDS_BITS = 7, GROUP_LDS_ENTRIES = 1u << GROUP_LDS_BITS, GROUP_LDS_KEYS = 64;

// The 64-bit hash of a value's units: FNV-1a over the units, then a finishing mix so that the upper half (the tag) and the lower
// bits (the first slot) both depend on every unit.  weak: GX_GROUP_WEAK_HASH's cut to the low 3 bits -- eight hashes in all, tag 0.
template <typename VP>
GX_WHERE_HD uint64_t group_hash(VP v, uint32_t n, bool weak) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t j = 0; j < n; ++j) h = (h ^ static_cast<uint64_t>(v[j])) * 0x100000001B3ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return weak ? (h & 7ull) : h;
}
GX_WHERE_HD uint32_t group_tag(uint64_t hash) { return static_cast<uint32_t>(hash >> 32); }
GX_WHERE_HD uint32_t group_first_slot(uint64_t hash, uint32_t n_slots) { return static_cast<uint32_t>(hash) & (n_slots - 1u); }   // (n_slots: a power of two)
GX_WHERE_HD uint64_t group_word(uint32_t tag, uint32_t line) { return (static_cast<uint64_t>(tag) << 32) | (static_cast<uint64_t>(line) + 1u); }   // (line < 2^32 - 1)
GX_WHERE_HD uint32_t group_word_line(uint64_t word) { return static_cast<uint32_t>(word) - 1u; }

// The table's slots: a power of two >= max(64, 2 * max_keys); max_keys <= 2^30, so at most 2^31.
inline uint32_t group_slots(uint64_t max_keys) {
    uint32_t s = 64;
    while (static_cast<uint64_t>(s) < 2u * max_keys) s <<= 1;
    return s;
}

// key equality: the same number of units and the same units
template <typename AP, typename BP>
GX_WHERE_HD bool group_same_key(AP a, uint32_t an, BP b, uint32_t bn) {
    return an == bn && where_same(a, b, an);
}

// Find-or-insert of the value v[0, vn) of line `line`.  Returns the key's slot, or GROUP_NONE when every slot holds another key.
//   table.load(slot)         the slot's word
//   table.claim(slot, word)  writes `word` if the slot is empty; returns what the slot held before (0: the claim won)
//   same(rep_line, v, vn)    is line rep_line's key the value v[0, vn)?  (reads rep_line's key from the batch)
// On the device claim is a 64-bit compare-and-swap on global memory, on the host a plain compare-and-store.
template <typename Table, typename VP, typename Same>
GX_WHERE_HD uint32_t group_find_or_insert(Table& table, uint32_t n_slots, uint64_t hash, uint32_t line, VP v, uint32_t vn, Same&& same) {
    const uint32_t tag = group_tag(hash);
    const uint64_t word = group_word(tag, line);
    uint32_t slot = group_first_slot(hash, n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        uint64_t cur = table.load(slot);
        if (cur == 0) {
            cur = table.claim(slot, word);
            if (cur == 0) return slot;   // this line represents the key
        }
        // (cur != 0 from here on and for ever: the slot is full)
        if (group_tag(cur) == tag && same(group_word_line(cur), v, vn)) return slot;
        slot = (slot + 1u) & (n_slots - 1u);
    }
    return GROUP_NONE;
}

// The table on the host: plain words.
struct GroupHostTable {
    uint64_t* words;
    uint64_t load(uint32_t slot) const { return words[slot]; }
    uint64_t claim(uint32_t slot, uint64_t word) {
        const uint64_t was = words[slot];
        if (was == 0) words[slot] = word;
        return was;
    }
};

// The parts as the kernel reads them, built by the host (gx_api.cpp: group_image) and copied to LDS by every workgroup: ext[] holds the
// extractions that have a part, ascending, searched with where_find (StatsHead's scheme; a part per extraction makes first[] unnecessary).
struct GroupPart {
    uint16_t key_group;
    uint16_t value_group;   // GROUP_NO_VALUE: count only
};
struct GroupHead {
    uint32_t n_parts, flags, has_values;
    uint32_t formats;                // != 0: some fmt[] is not LONG -- the host launches the build pass's instantiation that reads them
    uint32_t ext[GROUP_MAX_PARTS];
    GroupPart part[GROUP_MAX_PARTS];
    uint8_t fmt[GROUP_MAX_PARTS];    // part[e].value_group's packed number format (gx_number.hpp), 0 = LONG
};
static_assert(sizeof(GroupPart) == 4 && sizeof(GroupHead) % 16 == 0, "the head is copied in 16-byte words");

// A slot's words beside the table, all 64-bit and all zero when nothing was added, so that one memset prepares them and every merge
// is an unsigned add or an unsigned maximum: the lines, the FIRST line as ~line (the maximum of ~line is the minimum of line; 0: none),
// and -- when a part has a value group -- StatsAcc's three counts, lo, hi, and min / max in an order-preserving unsigned form.
enum : uint32_t { GROUP_W_LINES = 0, GROUP_W_FIRST, GROUP_HEAD_WORDS };
enum : uint32_t { GROUP_S_NUMBERS = 0, GROUP_S_UNSET, GROUP_S_NOT_NUMBERS, GROUP_S_MIN, GROUP_S_MAX, GROUP_S_LO, GROUP_S_HI, GROUP_S_SPARE, GROUP_STATS_WORDS };

GX_WHERE_HD uint64_t group_first_word(uint32_t line) { return 0xFFFFFFFFull - line; }           // (line < 2^32 - 1: never 0)
GX_WHERE_HD uint32_t group_first_line(uint64_t word) { return static_cast<uint32_t>(0xFFFFFFFFull - word); }
// int64 -> uint64 keeping the order; a minimum is kept as the maximum of the complement
GX_WHERE_HD uint64_t group_max_word(int64_t v) { return static_cast<uint64_t>(v) ^ 0x8000000000000000ull; }
GX_WHERE_HD uint64_t group_min_word(int64_t v) { return ~group_max_word(v); }
GX_WHERE_HD int64_t group_max_of(uint64_t w) { return static_cast<int64_t>(w ^ 0x8000000000000000ull); }
GX_WHERE_HD int64_t group_min_of(uint64_t w) { return group_max_of(~w); }

// A key's gx_measure_stats from its slot's stats words (the field order of gx_measure_stats: lines, numbers, unset, not_numbers, min,
// max, sum_lo, sum_hi), as eight 64-bit words.
GX_WHERE_HD void group_stats_out(const uint64_t* w, uint64_t* out) {
    const uint64_t numbers = w[GROUP_S_NUMBERS];
    out[0] = numbers + w[GROUP_S_UNSET] + w[GROUP_S_NOT_NUMBERS];
    out[1] = numbers;
    out[2] = w[GROUP_S_UNSET];
    out[3] = w[GROUP_S_NOT_NUMBERS];
    out[4] = static_cast<uint64_t>(numbers ? group_min_of(w[GROUP_S_MIN]) : STATS_INT64_MAX);
    out[5] = static_cast<uint64_t>(numbers ? group_max_of(w[GROUP_S_MAX]) : STATS_INT64_MIN);
    uint64_t lo = 0;
    int64_t hi = 0;
    stats_sum128(w[GROUP_S_LO], static_cast<int64_t>(w[GROUP_S_HI]), &lo, &hi);
    out[6] = lo;
    out[7] = static_cast<uint64_t>(hi);
}

}  // namespace gx
