// gx_where_dev.hpp -- device helpers that the passes over a finished batch's captured values share (gx_where.hip: select by value;
// gx_stats.hip: summarise values): a group's capture offsets in any row format, and "every term of the line's extraction holds",
// stated once (the rule of a single term: gx_where.hpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_layout.hpp"
#include "gx_number.hpp"
#include "gx_where.hpp"

namespace gx {

// a group's capture offsets in any row format: dense rows int32 caps[i][slots], compact rows behind the id in the line's result row
template <RowFormat F>
__device__ __forceinline__ void pair_of(const void* ids, const int32_t* caps, uint64_t i, uint32_t row_units, uint32_t slots, uint32_t g, int32_t& pb,
                                        int32_t& pe) {
    if (F == ROWS_DENSE) {
        const int32_t* row = caps + i * static_cast<uint64_t>(slots) + 2u * g;
        pb = row[0];
        pe = row[1];
    } else if (F == ROWS_U16) {
        const uint16_t* row = static_cast<const uint16_t*>(ids) + i * row_units + 1u + 2u * g;
        pb = decode_offset(F, row[0]);
        pe = decode_offset(F, row[1]);
    } else {
        const uint8_t* row = static_cast<const uint8_t*>(ids) + i * row_units + 1u + 2u * g;
        pb = decode_offset(F, row[0]);
        pe = decode_offset(F, row[1]);
    }
}

// Line i, whose outcome oc is a matched extraction: does every term of that extraction hold?  head / lits: the term image (WhereHead,
// then the literals) in LDS; line: the line's first code unit; line_units: its length (0 for a line the call refuses anyway -- then no
// value is looked at).  An extraction without terms holds.  The terms are tested in the caller's order and a line leaves at its first
// term that fails; a pair that names no value (where_pair_set) is never dereferenced.  NUM: an integer term parses its value under
// the format beside it (WhereHead::fmt); without it every one is Long.parseLong's, the code of a call that names LONG groups alone.
template <RowFormat F, typename UNIT, bool NUM>
__device__ __forceinline__ bool where_line_holds(const WhereHead* head, const UNIT* lits, uint32_t oc, const void* ids, const int32_t* caps, uint64_t i,
                                                 uint32_t row_units, uint32_t slots, const UNIT* line, uint64_t line_units) {
    const uint32_t n_ext = head->n_ext;
    const uint32_t e = where_find(head->ext, n_ext, oc);
    if (e >= n_ext) return true;
    bool kept = true;
    const uint32_t t1 = head->first[e + 1u];
    for (uint32_t t = head->first[e]; kept && t < t1; ++t) {   // (in the caller's order; a line leaves at its first term that fails)
        const WhereTerm& m = head->term[t];
        int32_t pb, pe;
        pair_of<F>(ids, caps, i, row_units, slots, m.group, pb, pe);
        bool holds = false;
        if (where_pair_set(pb, pe, line_units))
            holds = number_where_test<NUM>(NUM ? head->fmt[t] : 0u, m.op, line + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), lits + m.lit_at,
                                           m.lit_len, m.number);
        kept = kept && (holds != (m.negate != 0));
    }
    return kept;
}

}  // namespace gx
