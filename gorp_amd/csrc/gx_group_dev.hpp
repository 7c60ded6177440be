// gx_group_dev.hpp -- device code the passes of gx_group_lines (gx_group.hip) and of gx_top_groups (gx_top_groups.hip) share: how a
// pass finds the key of a line in a finished batch; and the workgroup's LDS table of the slots it adds to, which the pair pass
// (gx_pairs.hip) keys by pair slot.
#pragma once
#include <cstdint>

#include "gx_group.hpp"
#include "gx_outcome.hpp"
#include "gx_where_dev.hpp"

namespace gx {

// a finished batch as the passes read it
template <typename OFF, RowFormat F, typename UNIT>
struct GroupBatch {
    const void* ids;
    const int32_t* caps;
    uint32_t row_units, slots, K;
    const OFF* off;
    const UNIT* data;
    const GroupHead* gh;   // in LDS

    // The key of line r, which HAS one (its outcome has a part and the part's key pair is set: it is in the table, or about to be).
    __device__ __forceinline__ const UNIT* key_of(uint32_t r, uint32_t& units) const {
        const uint32_t oc = outcome_of(id_of<F>(ids, r, row_units), K);
        const uint32_t e = where_find(gh->ext, gh->n_parts, oc);
        int32_t pb, pe;
        pair_of<F>(ids, caps, r, row_units, slots, gh->part[e < gh->n_parts ? e : 0u].key_group, pb, pe);
        units = static_cast<uint32_t>(pe - pb);
        return data + static_cast<uint64_t>(off[r]) + static_cast<uint32_t>(pb);
    }
};

// what one slot receives: GROUP_HEAD_WORDS words at `head`, GROUP_STATS_WORDS at `stats` (with values); zeros are not sent.  The build
// passes of gx_group.hip and gx_bucket.hip add it to a workgroup's LDS entry or to the slot's words in global memory.
struct GroupAdd {
    uint64_t lines, first, numbers, unset, not_numbers, mn, mx, lo, hi;
};
__device__ __forceinline__ void group_add(unsigned long long* head, unsigned long long* stats, bool values, const GroupAdd& a) {
    typedef unsigned long long u64;
    atomicAdd(head + GROUP_W_LINES, static_cast<u64>(a.lines));
    atomicMax(head + GROUP_W_FIRST, static_cast<u64>(a.first));
    if (values) {
        if (a.unset) atomicAdd(stats + GROUP_S_UNSET, static_cast<u64>(a.unset));
        if (a.not_numbers) atomicAdd(stats + GROUP_S_NOT_NUMBERS, static_cast<u64>(a.not_numbers));
        if (a.numbers) {
            atomicAdd(stats + GROUP_S_NUMBERS, static_cast<u64>(a.numbers));
            atomicAdd(stats + GROUP_S_LO, static_cast<u64>(a.lo));
            atomicAdd(stats + GROUP_S_HI, static_cast<u64>(a.hi));
            atomicMax(stats + GROUP_S_MIN, static_cast<u64>(a.mn));
            atomicMax(stats + GROUP_S_MAX, static_cast<u64>(a.mx));
        }
    }
}

// The entry of `slot` in the workgroup's LDS table (keys[GROUP_LDS_ENTRIES], GROUP_NONE: free), inserted if it is new and the table
// still takes keys; GROUP_NONE: the table is full, add to global memory.  At most GROUP_LDS_KEYS entries are ever claimed (a claim is
// reserved in *used first), so a free entry ends every probe sequence and the loop is bounded by the table besides.
__device__ __forceinline__ uint32_t group_lds_entry(uint32_t* keys, uint32_t* used, uint32_t slot) {
    uint32_t e = (slot * 0x9E3779B1u) >> (32u - GROUP_LDS_BITS);
    bool reserved = false;
    for (uint32_t probe = 0; probe < GROUP_LDS_ENTRIES; ++probe) {
        uint32_t k = __hip_atomic_load(keys + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == slot) return e;
        if (k == GROUP_NONE) {
            if (!reserved) {
                if (__hip_atomic_load(used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= GROUP_LDS_KEYS) return GROUP_NONE;
                if (atomicAdd(used, 1u) >= GROUP_LDS_KEYS) return GROUP_NONE;
                reserved = true;
            }
            k = atomicCAS(keys + e, GROUP_NONE, slot);
            // (k == slot: another wave claimed this very slot's entry meanwhile.  The reservation is not handed back, so the table may
            // refuse new slots a little before it holds GROUP_LDS_KEYS; those add to global memory directly -- capacity, never results.)
            if (k == GROUP_NONE || k == slot) return e;
        }
        e = (e + 1u) & (GROUP_LDS_ENTRIES - 1u);
    }
    return GROUP_NONE;
}

}  // namespace gx
