// gx_utf8.hip -- UTF-8 lines as the Strings Java would see (gx_batch_opts.utf8, gx_utf8_to_utf16): the decoding rule of
// gx_utf8.hpp on the device.  The reference never sees bytes: its callers hand Gorp.extract a java.lang.String, and the one
// place it decodes itself is new InputStreamReader(in, "UTF-8").  The byte batch kernels are right for every ASCII-only line;
// the passes here make the UTF-16 code units of the OTHER lines, for the per-line walk on units (gx_kernels.hip:
// k_extract_listed), and take its capture offsets back to bytes.
//
//   flag sweep   (only when the caller brings no line flags) aligned 16-byte loads over [offsets[0], offsets[n]); a chunk that
//                holds a byte >= 0x80 finds its line(s) by binary search in the offsets and stores flags[line] = 1 (plain stores);
//   count        units per line (0 for an unflagged line), then gx_scan.hpp -> unit offsets; beside them the list of the flagged
//                lines' numbers, so that the walk gives every lane a flagged line however few there are;
//   write        the units of every flagged line and, beside each, the byte its item starts at (so that offsets go back to bytes
//                by a gather);
//   offsets back to bytes   the rows of flagged lines, all three row formats.
// Count and write share one body: 16 lanes take a line, 256 bytes a pass, one aligned 16-byte load per lane; the three bytes either
// side of a lane's sixteen come from its neighbours by __shfl, and from a few byte loads at the group's two edges.  A wave
// looks at the flags of 64 lines at once (one coalesced load, one ballot) and hands its four groups the flagged ones, so a batch
// with few flagged lines costs a read of its flags.  Bytes outside the batch are never read, bytes outside a line never looked at.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_scan.hpp"
#include "gx_utf8.hpp"

namespace gx {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed)) UnalignedStore16 { u32x4 v; };

// the 16 bytes at address a (16-byte aligned); bytes outside [lo, hi) are not read and come as 0
__device__ __forceinline__ u32x4 load16_within(uintptr_t a, uintptr_t lo, uintptr_t hi) {
    if (a >= lo && a + 16 <= hi) return *reinterpret_cast<const u32x4*>(a);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (a + r >= lo && a + r < hi) w[r >> 2] |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(a + r)) << ((r & 3) * 8);
    return u32x4{w[0], w[1], w[2], w[3]};
}

// the line that holds position pos: off[line] <= pos < off[line + 1] (pos inside the batch)
template <typename OFF>
__device__ __forceinline__ uint64_t line_of(const OFF* __restrict__ off, uint64_t n, uint64_t pos) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (static_cast<uint64_t>(off[mid]) <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename OFF>
__global__ void __launch_bounds__(256) k_utf8_flags(const uint8_t* __restrict__ data, const OFF* __restrict__ off, uint64_t n, uint8_t* __restrict__ flags) {
    const uint64_t first = off[0], last = off[n];
    const uintptr_t lo = reinterpret_cast<uintptr_t>(data + first), hi = reinterpret_cast<uintptr_t>(data + last);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u * 16u;
    for (uintptr_t a = (lo & ~static_cast<uintptr_t>(15)) + (static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x) * 16u; a < hi; a += stride) {
        const u32x4 v = load16_within(a, lo, hi);
        if (((v.x | v.y | v.z | v.w) & 0x80808080u) == 0u) continue;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint64_t line_end = 0;   // (the end of the line flagged last: its later bytes need no search)
        for (int r = 0; r < 16; ++r) {
            if (!((w[r >> 2] >> ((r & 3) * 8)) & 0x80u)) continue;
            const uint64_t pos = first + (a + r - lo);
            if (pos < line_end) continue;
            const uint64_t line = line_of(off, n, pos);
            flags[line] = 1;
            line_end = off[line + 1];
        }
    }
}

// WRITE = false: counts[line] = the line's units (0: not flagged), *flagged += the flagged lines; list (optional): their numbers,
// a wave's own in order behind one atomicAdd per 64 lines that hold any.
// WRITE = true: the units of every flagged line at units[unit_off[line] ..), and unit_byte (optional) beside them.
// flags == nullptr: every line is flagged.
template <typename OFF, bool WRITE>
__global__ void __launch_bounds__(256) k_utf8_lines(const uint8_t* __restrict__ data, const OFF* __restrict__ off, uint64_t n, const uint8_t* __restrict__ flags,
                                                    uint32_t* __restrict__ counts, unsigned long long* __restrict__ flagged, uint32_t* __restrict__ status,
                                                    uint64_t* __restrict__ list, const uint64_t* __restrict__ unit_off, uint16_t* __restrict__ units, uint32_t* __restrict__ unit_byte) {
    const uint32_t lane = threadIdx.x & 63u, gl = lane & 15u, group = lane >> 4;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(data + off[0]), hi = reinterpret_cast<uintptr_t>(data + off[n]);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    uint32_t n_flagged = 0;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t mine = i0 + lane;
        const bool flag = mine < n && (!flags || flags[mine] != 0);
        if (!WRITE && mine < n && !flag) counts[mine] = 0u;
        uint64_t todo = __ballot(flag);
        if (!WRITE && list) {
            if (todo) {
                unsigned long long base = 0;
                if (lane == 0u) base = atomicAdd(flagged, static_cast<unsigned long long>(__popcll(todo)));
                base = __shfl(base, 0);
                if (flag) list[base + static_cast<uint32_t>(__popcll(todo & ((1ull << lane) - 1ull)))] = mine;
            }
        } else {
            n_flagged += static_cast<uint32_t>(__popcll(todo));
        }
        while (todo) {
            // the wave's next four flagged lines, one per group
            int bit = -1;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                if (!todo) break;
                if (q == group) bit = __ffsll(static_cast<unsigned long long>(todo)) - 1;
                todo &= todo - 1u;
            }
            if (bit < 0) continue;
            const uint64_t line = i0 + static_cast<uint32_t>(bit);
            const uint64_t beg = off[line], end = off[line + 1];
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(data + beg), a_end = reinterpret_cast<uintptr_t>(data + end);
            uint64_t run = WRITE ? unit_off[line] : 0;   // units of the line before this pass
            for (uintptr_t c = a0 & ~static_cast<uintptr_t>(15); c < a_end; c += 256u) {
                const uintptr_t ca = c + gl * 16u;
                const bool live = ca < a_end;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (live) v = load16_within(ca, lo, hi);
                uint32_t prev = static_cast<uint32_t>(__shfl_up(static_cast<int>(v.w), 1, 16));
                uint32_t next = static_cast<uint32_t>(__shfl_down(static_cast<int>(v.x), 1, 16));
                // the group's edges: the bytes the neighbouring pass holds, as far as they are the line's
                const auto byte_at = [](uint64_t a) { return *reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(a)); };
                if (gl == 0u) prev = utf8_edge_prev(byte_at, ca, a0, a_end);
                if (gl == 15u) next = utf8_edge_next(byte_at, ca, a_end);
                const bool whole = ca >= a0 && ca + 16u <= a_end;
                const bool ascii = whole && ((v.x | v.y | v.z | v.w) & 0x80808080u) == 0u;
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
                uint32_t cnt = 0;
                Utf8Window x;
                if (ascii) cnt = 16u;
                else if (live) {
                    x = utf8_make_window(d, prev, next, ca, a0, a_end);
                    cnt = utf8_chunk_units(x, [](int, uint32_t, uint16_t) {});
                }
                // the lane's first unit: the units of the lanes before it in the group
                uint32_t inc = cnt;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const uint32_t o = static_cast<uint32_t>(__shfl_up(static_cast<int>(inc), d, 16));
                    if (gl >= static_cast<uint32_t>(d)) inc += o;
                }
                const uint32_t pass_units = static_cast<uint32_t>(__shfl(static_cast<int>(inc), 15, 16));
                if (WRITE) {
                    uint64_t at = run + inc - cnt;
                    const uint32_t byte0 = static_cast<uint32_t>(ca - a0);   // (wraps for the bytes before the line, which write nothing)
                    if (ascii) {
                        uint32_t pair[8];
                        utf8_widen_ascii(d, pair);
                        UnalignedStore16* dst = reinterpret_cast<UnalignedStore16*>(units + at);
                        dst[0].v = u32x4{pair[0], pair[1], pair[2], pair[3]};
                        dst[1].v = u32x4{pair[4], pair[5], pair[6], pair[7]};
                        if (unit_byte) {
#pragma unroll
                            for (uint32_t j = 0; j < 16u; ++j) unit_byte[at + j] = byte0 + j;
                        }
                    } else if (live) {
                        utf8_chunk_units(x, [&](int j, uint32_t, uint16_t unit) {
                            units[at] = unit;
                            if (unit_byte) unit_byte[at] = byte0 + static_cast<uint32_t>(j);
                            ++at;
                        });
                    }
                }
                run += pass_units;
            }
            if (!WRITE && gl == 0u) {
                if (run > 0xFFFFFFFFull) { atomicOr(status, 1u); run = 0; }   // (a line of 4 G units: refused by the host)
                counts[line] = static_cast<uint32_t>(run);
            }
        }
    }
    if (!WRITE && lane == 0u && n_flagged) atomicAdd(flagged, static_cast<unsigned long long>(n_flagged));
}

// unit offsets (u64, the scan's) in the width the caller's offsets have
__global__ void __launch_bounds__(256) k_utf8_offsets32(const uint64_t* __restrict__ in, uint64_t n1, uint32_t* __restrict__ out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n1; i += stride) out[i] = static_cast<uint32_t>(in[i]);
}

// The rows of flagged lines hold offsets in code units (k_extract_listed wrote them): every set offset u becomes the byte of the
// item unit u starts in; u = the line's units becomes its length in bytes.  One lane per line.
template <typename OFF, RowFormat F>
__global__ void __launch_bounds__(256) k_utf8_offsets_to_bytes(int32_t* __restrict__ caps, uint8_t* __restrict__ rows, unsigned long long* __restrict__ overflow,
                                                               uint32_t slots, uint64_t n, const uint8_t* __restrict__ flags, const OFF* __restrict__ off,
                                                               const uint64_t* __restrict__ unit_off, const uint32_t* __restrict__ unit_byte) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!flags[i]) continue;
        const uint64_t u0 = unit_off[i], n_units = unit_off[i + 1] - u0;
        const uint64_t len = static_cast<uint64_t>(off[i + 1]) - static_cast<uint64_t>(off[i]);
        uint32_t clipped = 0;
        for (uint32_t t = 0; t < slots; ++t) {
            uint32_t unit;
            if (F == ROWS_DENSE) unit = static_cast<uint32_t>(caps[i * slots + t]);
            else if (F == ROWS_U16) unit = reinterpret_cast<const uint16_t*>(rows + i * row_bytes(F, slots))[1u + t];
            else unit = rows[i * row_bytes(F, slots) + 1u + t];
            const int32_t v = decode_offset(F, unit);
            if (v < 0) continue;
            const uint64_t b = static_cast<uint64_t>(v) < n_units ? unit_byte[u0 + static_cast<uint64_t>(v)] : len;
            const RowUnit e = encode_offset(F, static_cast<int32_t>(b > 0x7FFFFFFFull ? 0x7FFFFFFFull : b));
            clipped += e.clipped;
            if (F == ROWS_DENSE) caps[i * slots + t] = static_cast<int32_t>(e.unit);
            else if (F == ROWS_U16) reinterpret_cast<uint16_t*>(rows + i * row_bytes(F, slots))[1u + t] = static_cast<uint16_t>(e.unit);
            else rows[i * row_bytes(F, slots) + 1u + t] = static_cast<uint8_t>(e.unit);
        }
        if (clipped && overflow) atomicAdd(overflow, static_cast<unsigned long long>(clipped));
    }
}

constexpr size_t up16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

unsigned line_blocks(uint64_t n) {
    const uint64_t need = (n + 255) / 256;
    return static_cast<unsigned>(need < 1 ? 1 : need > 256u * 16u ? 256u * 16u : need);
}

}  // namespace

size_t utf8_workspace_bytes(uint64_t n) { return up16(n + 16) + up16((n + 1) * 4) + up16((n + 1) * 8) + up16(n * 8) + scan_sums_bytes(n) + 32; }

Utf8Ws utf8_workspace(void* ws, uint64_t n) {
    Utf8Ws w{};
    uint8_t* p = static_cast<uint8_t*>(ws);
    w.unit_off = reinterpret_cast<uint64_t*>(p); p += up16((n + 1) * 8);
    w.list = reinterpret_cast<uint64_t*>(p); p += up16(n * 8);
    w.block_sums = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n);
    w.flagged = reinterpret_cast<unsigned long long*>(p);
    w.status = reinterpret_cast<uint32_t*>(p + 8); p += 32;
    w.counts = reinterpret_cast<uint32_t*>(p); p += up16((n + 1) * 4);
    w.flags = p;
    return w;
}

hipError_t launch_utf8_flags(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, uint8_t* flags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(flags, 0, n, stream);
    if (e != hipSuccess) return e;
    const dim3 grid(256u * 8u), block(256);
    if (offsets64) hipLaunchKernelGGL((k_utf8_flags<uint64_t>), grid, block, 0, stream, data, static_cast<const uint64_t*>(offsets), n, flags);
    else hipLaunchKernelGGL((k_utf8_flags<uint32_t>), grid, block, 0, stream, data, static_cast<const uint32_t*>(offsets), n, flags);
    return hipGetLastError();
}

hipError_t launch_utf8_count(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, const uint8_t* flags, const Utf8Ws& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.flagged, 0, 32, stream);
    if (e != hipSuccess) return e;
    if (n == 0) return hipMemsetAsync(w.unit_off, 0, 8, stream);
    const dim3 grid(line_blocks(n)), block(256);
    if (offsets64)
        hipLaunchKernelGGL((k_utf8_lines<uint64_t, false>), grid, block, 0, stream, data, static_cast<const uint64_t*>(offsets), n, flags, w.counts, w.flagged, w.status,
                           flags ? w.list : nullptr, nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL((k_utf8_lines<uint32_t, false>), grid, block, 0, stream, data, static_cast<const uint32_t*>(offsets), n, flags, w.counts, w.flagged, w.status,
                           flags ? w.list : nullptr, nullptr, nullptr, nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.counts, n, w.block_sums, w.unit_off, stream);
}

hipError_t launch_utf8_write(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, const uint8_t* flags, const uint64_t* unit_off, uint16_t* units,
                             uint32_t* unit_byte, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(line_blocks(n)), block(256);
    if (offsets64)
        hipLaunchKernelGGL((k_utf8_lines<uint64_t, true>), grid, block, 0, stream, data, static_cast<const uint64_t*>(offsets), n, flags, nullptr, nullptr, nullptr, nullptr,
                           unit_off, units, unit_byte);
    else
        hipLaunchKernelGGL((k_utf8_lines<uint32_t, true>), grid, block, 0, stream, data, static_cast<const uint32_t*>(offsets), n, flags, nullptr, nullptr, nullptr, nullptr,
                           unit_off, units, unit_byte);
    return hipGetLastError();
}

hipError_t launch_utf8_offsets32(const uint64_t* unit_off, uint64_t n, uint32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_utf8_offsets32, dim3(line_blocks(n + 1)), dim3(256), 0, stream, unit_off, n + 1, out);
    return hipGetLastError();
}

hipError_t launch_utf8_offsets_to_bytes(const GxDev& dev, const GxBatch& b, const uint8_t* flags, const uint64_t* unit_off, const uint32_t* unit_byte,
                                        hipStream_t stream) {
    const uint32_t slots = 2u * static_cast<uint32_t>(dev.max_groups);
    if (b.n == 0 || slots == 0 || b.match_only) return hipSuccess;
    const RowFormat f = row_format(b.packed != nullptr, b.narrow != 0);
    const dim3 grid(line_blocks(b.n)), block(256);
    uint8_t* rows = reinterpret_cast<uint8_t*>(b.packed);
#define GX_TO_BYTES(OFF, F) hipLaunchKernelGGL((k_utf8_offsets_to_bytes<OFF, F>), grid, block, 0, stream, b.caps, rows, b.overflow, slots, b.n, flags, \
                                               static_cast<const OFF*>(b.offsets), unit_off, unit_byte)
    if (b.offsets64) { if (f == ROWS_DENSE) GX_TO_BYTES(uint64_t, ROWS_DENSE); else if (f == ROWS_U16) GX_TO_BYTES(uint64_t, ROWS_U16); else GX_TO_BYTES(uint64_t, ROWS_U8); }
    else { if (f == ROWS_DENSE) GX_TO_BYTES(uint32_t, ROWS_DENSE); else if (f == ROWS_U16) GX_TO_BYTES(uint32_t, ROWS_U16); else GX_TO_BYTES(uint32_t, ROWS_U8); }
#undef GX_TO_BYTES
    return hipGetLastError();
}

}  // namespace gx
