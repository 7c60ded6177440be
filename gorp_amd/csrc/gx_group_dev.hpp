// gx_group_dev.hpp -- device code the passes of gx_group_lines (gx_group.hip) and of gx_top_groups (gx_top_groups.hip) share: how a
// pass finds the key of a line in a finished batch.
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

}  // namespace gx
