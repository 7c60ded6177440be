// gx_outcome.hpp -- device helpers that the passes over a finished batch's outcomes share (gx_select.hip: count and select;
// gx_partition.hip: partition): the outcome index of an id, the id of a line in any row format, and the two pieces of a copy
// that writes aligned 16-byte chunks from a source that sits elsewhere in its own.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_layout.hpp"

namespace gx {

// The outcome index over K extractions: id in [0, K) -> id; -1 -> K; -2-k -> K + 1 + k; any other value (a row nobody wrote)
// -> 2K + 1, counted and never selected.
__device__ __forceinline__ uint32_t outcome_of(int32_t id, uint32_t K) {
    const int64_t k = static_cast<int64_t>(K), v = id;
    if (v >= 0) return v < k ? static_cast<uint32_t>(v) : 2u * K + 1u;
    if (v == -1) return K;
    return v >= -1 - k ? K + 1u + static_cast<uint32_t>(-2 - v) : 2u * K + 1u;
}

template <RowFormat F>
__device__ __forceinline__ int32_t id_of(const void* ids, uint64_t i, uint32_t row_units) {
    if (F == ROWS_U8) return decode_id(F, static_cast<const uint8_t*>(ids)[i * row_units]);
    if (F == ROWS_U16) return decode_id(F, static_cast<const uint16_t*>(ids)[i * row_units]);
    return static_cast<const int32_t*>(ids)[i];
}

// the 16 bytes at p (16-byte aligned); bytes outside [lo, hi) are not read (a buffer may end at the end of a page) and come as 0
__device__ __forceinline__ uint4 load16_within(const uint8_t* p, uintptr_t lo, uintptr_t hi) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a >= lo && a + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        uint32_t b = 0;
        if (a + r >= lo && a + r < hi) b = static_cast<uint32_t>(p[r]) << ((r & 3) * 8);
        if (r < 4) w0 |= b; else if (r < 8) w1 |= b; else if (r < 12) w2 |= b; else w3 |= b;
    }
    return make_uint4(w0, w1, w2, w3);
}

// bytes [r, r + 4) of the eight bytes lo | hi (v_alignbyte)
__device__ __forceinline__ uint32_t ab(uint32_t hi, uint32_t lo, uint32_t r) { return __builtin_amdgcn_alignbyte(hi, lo, r); }

}  // namespace gx
