// gx_select.hip -- what a caller does with the outcomes of a finished batch, on the device: count the lines per outcome and
// select lines (their text, their result rows, their line numbers) by outcome.  The reference's caller sees every outcome in
// its own loop (README.md:26,63-79): a null result is a line no extraction matched, an ExtractionException a line whose
// capture regexp disagreed with the automaton, a result carries the id of its extraction (core/Gorp.java:159-186).  In bulk
// the outcomes are a column of ids in device memory; these passes keep the rest of that loop there too.
//
// The outcome index over K extractions (outcome_of, gx_outcome.hpp): id in [0, K) -> id; -1 -> K; -2-k -> K + 1 + k; any other value
// (a row nobody wrote) -> 2K + 1, counted and never selected.
//
// Three passes.  Flags (k_select_flags): one read of the id column and the offsets; per line "kept" and the kept length; the
// histogram of outcomes in LDS, left as one slab per workgroup and summed by k_select_sum (no atomics in global memory: on one
// cache line they take their turns at 11 ns apiece).  Scan (gx_scan.hpp) of both columns.  Copy (k_select_copy): a wave owns 64
// consecutive lines; their kept lines form runs that are contiguous in the source and in the destination, and a run leaves as
// 16-byte stores to aligned destination addresses, its source realigned in registers.  DESIGN.md section 5.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_outcome.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t sel_smem[];

// SELECT = false: the histogram alone (gx_count_outcomes).  lds_bins != 0: the 2K + 2 bins (and the want mask behind them) are in
// LDS and leave as slab[blockIdx.x][bins]; 0 (more bins than LDS takes): every wave adds to counts[] in global memory.
template <typename OFF, RowFormat F, bool SELECT>
__global__ void __launch_bounds__(256) k_select_flags(const void* __restrict__ ids, uint32_t row_units, uint32_t K, uint64_t n, const OFF* __restrict__ off,
                                                      const uint8_t* __restrict__ want, uint8_t* __restrict__ flags, uint32_t* __restrict__ klen,
                                                      uint32_t* __restrict__ slab, unsigned long long* __restrict__ counts, uint32_t lds_bins,
                                                      uint32_t* __restrict__ status) {
    const uint32_t bins = 2u * K + 2u;
    uint32_t* hist = sel_smem;
    const uint8_t* want_l = want;
    if (lds_bins) {
        for (uint32_t q = threadIdx.x; q < bins; q += 256u) hist[q] = 0u;
        if (SELECT) {
            uint8_t* w = reinterpret_cast<uint8_t*>(hist + bins);
            for (uint32_t q = threadIdx.x; q < bins - 1u; q += 256u) w[q] = want[q];
            want_l = w;
        }
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        const uint32_t oc = valid ? outcome_of(id_of<F>(ids, i, row_units), K) : 0xFFFFFFFFu;
        if (SELECT) {
            if (valid) {
                const bool kept = oc <= 2u * K && want_l[oc] != 0;
                const uint64_t len = static_cast<uint64_t>(off[i + 1]) - static_cast<uint64_t>(off[i]);
                if (len > 0xFFFFFFFFull) atomicOr(status, 1u);   // (a line of 4 G code units: refused by the host)
                flags[i] = kept ? 1 : 0;
                klen[i] = kept ? static_cast<uint32_t>(len) : 0u;
            }
        }
        // one addition per distinct outcome of the wave's 64 lines (mostly two or three)
        uint64_t todo = __ballot(valid);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(todo))) - 1u;
            const uint32_t v = static_cast<uint32_t>(__shfl(static_cast<int>(oc), static_cast<int>(l)));
            const uint64_t m = __ballot(oc == v);
            if (lane == l) {
                if (lds_bins) atomicAdd(&hist[v], static_cast<uint32_t>(__popcll(m)));
                else atomicAdd(counts + v, static_cast<unsigned long long>(__popcll(m)));
            }
            todo &= ~m;
        }
    }
    if (lds_bins) {
        __syncthreads();
        uint32_t* mine = slab + static_cast<uint64_t>(blockIdx.x) * bins;
        for (uint32_t q = threadIdx.x; q < bins; q += 256u) mine[q] = hist[q];
    }
}

// counts[bin] = sum over the workgroups' slabs; one workgroup per bin
__global__ void __launch_bounds__(256) k_select_sum(const uint32_t* __restrict__ slab, uint32_t blocks, uint32_t bins, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long wsum[4];
    unsigned long long t = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) t += slab[static_cast<uint64_t>(b) * bins + blockIdx.x];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(v)); }
__device__ __forceinline__ uint64_t uni(uint64_t v) {
    return (static_cast<uint64_t>(uni(static_cast<uint32_t>(v >> 32))) << 32) | static_cast<uint64_t>(uni(static_cast<uint32_t>(v)));
}
__device__ __forceinline__ uint64_t lane_value(uint64_t v, uint32_t l) {
    return static_cast<uint64_t>(__shfl(static_cast<unsigned long long>(v), static_cast<int>(l)));
}

// bytes [m, m + 16) of the 32 bytes a | b, m = 1 .. 15 and the same in every lane
__device__ __forceinline__ uint4 realign(const uint4& a, const uint4& b, uint32_t m) {
    const uint32_t r = m & 3u;
    switch (m >> 2) {
    case 0: return make_uint4(ab(a.y, a.x, r), ab(a.z, a.y, r), ab(a.w, a.z, r), ab(b.x, a.w, r));
    case 1: return make_uint4(ab(a.z, a.y, r), ab(a.w, a.z, r), ab(b.x, a.w, r), ab(b.y, b.x, r));
    case 2: return make_uint4(ab(a.w, a.z, r), ab(b.x, a.w, r), ab(b.y, b.x, r), ab(b.z, b.y, r));
    default: return make_uint4(ab(b.x, a.w, r), ab(b.y, b.x, r), ab(b.z, b.y, r), ab(b.w, b.z, r));
    }
}

// One run, the whole wave: len bytes from src to dst, every argument the same in all lanes.  The bytes before dst's first and
// behind its last 16-byte boundary leave as single bytes (at most 15 each: another wave may own the rest of those chunks, and
// nobody reads a chunk to write it back); everything between as aligned 16-byte stores, from two aligned 16-byte loads joined by
// v_alignbyte when the source sits elsewhere in its chunk.  Nothing outside [lo, hi) -- the batch's own bytes -- is read.
__device__ __forceinline__ void copy_run(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t lane, uintptr_t lo, uintptr_t hi) {
    uint32_t head = (16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (head > len) head = static_cast<uint32_t>(len);
    const uint64_t rest = len - head, body = rest >> 4;
    const uint32_t tail = static_cast<uint32_t>(rest & 15u);
    if (lane < head) dst[lane] = src[lane];
    else if (lane >= 16u && lane - 16u < tail) {
        const uint64_t at = head + (body << 4) + (lane - 16u);
        dst[at] = src[at];
    }
    if (body == 0) return;
    const uint8_t* sb = src + head;
    uint4* db = reinterpret_cast<uint4*>(dst + head);
    const uint32_t m = uni(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(sb) & 15u));
    const uint8_t* sa = sb - m;
    if (m == 0u) {
        const uint4* s4 = reinterpret_cast<const uint4*>(sa);
        uint64_t c = lane;
        for (; c + 64u < body; c += 128u) {
            const uint4 v0 = s4[c], v1 = s4[c + 64u];
            db[c] = v0;
            db[c + 64u] = v1;
        }
        if (c < body) db[c] = s4[c];
        return;
    }
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(sa);
    if (a0 >= lo && a0 + ((body + 1u) << 4) <= hi) {
        const uint4* s4 = reinterpret_cast<const uint4*>(sa);
        uint64_t c = lane;
        for (; c + 64u < body; c += 128u) {
            const uint4 a = s4[c], b = s4[c + 1u], d = s4[c + 64u], e = s4[c + 65u];
            db[c] = realign(a, b, m);
            db[c + 64u] = realign(d, e, m);
        }
        if (c < body) {
            const uint4 a = s4[c], b = s4[c + 1u];
            db[c] = realign(a, b, m);
        }
        return;
    }
    // (the batch's first or last run: source chunk 0 or chunk `body` sticks out of the batch's bytes; those two are read with
    // care, the chunks between them lie inside the run)
    const uint4* s4 = reinterpret_cast<const uint4*>(sa);
    auto chunk = [&](uint64_t j) -> uint4 { return (j == 0 || j == body) ? load16_within(sa + (j << 4), lo, hi) : s4[j]; };
    for (uint64_t c = lane; c < body; c += 64u) {
        const uint4 a = chunk(c), b = chunk(c + 1u);
        db[c] = realign(a, b, m);
    }
}

// A fixed-size column of the kept lines (result rows, capture rows, ids): `total` = kept lines x width units, the wave's lanes
// on consecutive units of the destination; tab[j] = the lane (= line of the tile) of the tile's j-th kept line.
template <typename UNIT>
__device__ __forceinline__ void copy_column(const void* src, void* dst, uint32_t width, uint64_t line0, uint64_t row0, uint32_t kept_lines,
                                            const uint8_t* tab, uint32_t lane) {
    const UNIT* s = static_cast<const UNIT*>(src) + line0 * width;
    UNIT* d = static_cast<UNIT*>(dst) + row0 * width;
    const uint32_t total = kept_lines * width;
    for (uint32_t t = lane; t < total; t += 64u) {
        const uint32_t j = t / width, c = t - j * width;
        d[t] = s[static_cast<uint32_t>(tab[j]) * width + c];
    }
}

struct SelectColumn {
    const void* src;
    void* dst;
    uint32_t width;       // units per line
    uint32_t unit_bytes;  // 1, 2 or 4
};

struct SelectCopy {
    const uint8_t* src;        // the batch's code units
    uint32_t unit_shift;       // 0: bytes, 1: UTF-16 code units
    uint64_t n;
    const uint8_t* flags;      // [n] kept
    const uint64_t* idx_off;   // [n + 1] kept lines before line i
    const uint64_t* dst_off;   // [n + 1] kept code units before line i
    uint32_t* out_index;       // optional
    uint8_t* out_bytes;        // optional
    void* out_offsets;         // optional, OFF[kept + 1]
    SelectColumn col[2];       // src == nullptr: none
};

template <typename OFF>
__global__ void __launch_bounds__(256) k_select_copy(SelectCopy a, const OFF* __restrict__ off) {
    __shared__ uint8_t tabs[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint8_t* tab = tabs[wave];
    const uint64_t n = a.n, tiles = (n + 63u) >> 6;
    const uint32_t sh = a.unit_shift;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(a.src) + (static_cast<uint64_t>(off[0]) << sh);
    const uintptr_t hi = reinterpret_cast<uintptr_t>(a.src) + (static_cast<uint64_t>(off[n]) << sh);
    OFF* out_off = static_cast<OFF*>(a.out_offsets);
    for (uint64_t tile = static_cast<uint64_t>(blockIdx.x) * 4u + wave; tile < tiles; tile += static_cast<uint64_t>(gridDim.x) * 4u) {
        const uint64_t i = (tile << 6) + lane;
        const bool valid = i < n;
        const bool kept = valid && a.flags[i] != 0;
        const uint64_t x0 = valid ? a.idx_off[i] : 0, d0 = valid ? a.dst_off[i] : 0, d1 = valid ? a.dst_off[i + 1] : 0;
        const uint64_t s0 = valid ? static_cast<uint64_t>(off[i]) : 0;
        if (out_off && i + 1 == n) out_off[a.idx_off[n]] = static_cast<OFF>(d1);
        const uint64_t M = __ballot(kept);
        if (M == 0) continue;
        if (kept) {
            if (a.out_index) a.out_index[x0] = static_cast<uint32_t>(i);
            if (out_off) out_off[x0] = static_cast<OFF>(d0);
        }
        if (a.out_bytes) {
            // the runs of kept lines: from a kept lane whose neighbour below is not kept, up to the next lane that is not
            uint64_t starts = M & ~(M << 1);
            while (starts) {
                const uint32_t r = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(starts))) - 1u;
                starts &= starts - 1;
                const uint64_t rest = ~(M >> r);   // (0: all 64 lanes are one run)
                const uint32_t e = rest ? r + static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(rest))) - 1u : 64u;   // first lane behind the run
                const uint64_t rs = uni(lane_value(s0, r)), rd = uni(lane_value(d0, r)), rd1 = uni(lane_value(d1, e - 1u));
                if (rd1 > rd) copy_run(a.src + (rs << sh), a.out_bytes + (rd << sh), (rd1 - rd) << sh, lane, lo, hi);
            }
        }
        if (a.col[0].src) {
            const uint64_t row0 = uni(lane_value(x0, 0));   // (the tile's first line exists; idx_off is what lies before it, kept or not)
            if (kept) tab[x0 - row0] = static_cast<uint8_t>(lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t kept_lines = static_cast<uint32_t>(__popcll(M));
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const SelectColumn& c = a.col[q];
                if (!c.src) continue;
                if (c.unit_bytes == 4u) copy_column<uint32_t>(c.src, c.dst, c.width, tile << 6, row0, kept_lines, tab, lane);
                else if (c.unit_bytes == 2u) copy_column<uint16_t>(c.src, c.dst, c.width, tile << 6, row0, kept_lines, tab, lane);
                else copy_column<uint8_t>(c.src, c.dst, c.width, tile << 6, row0, kept_lines, tab, lane);
            }
            // (the table is rewritten by the wave's next tile)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }

// workgroups of the flags pass (its slab has as many rows): one per 256 lines, 1 024 at most, fewer when the bins are many (the
// slab stays within a million entries, but no fewer than 64 workgroups)
uint32_t select_flag_blocks(uint64_t n, uint32_t bins) {
    const uint64_t by_lines = std::max<uint64_t>(1, (n + 255) / 256);
    const uint64_t by_slab = std::max<uint64_t>(64, (1u << 20) / std::max<uint32_t>(bins, 1u));
    return static_cast<uint32_t>(std::min<uint64_t>(std::min<uint64_t>(by_lines, by_slab), 1024));
}

}  // namespace

// select = false: the workspace of a count alone (counts, status, slab)
SelectWs select_workspace(void* ws, uint64_t n, uint32_t K, bool select) {
    const uint32_t bins = 2u * K + 2u;
    SelectWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.counts = reinterpret_cast<unsigned long long*>(take(static_cast<uint64_t>(bins) * 8));
    w.status = reinterpret_cast<uint32_t*>(take(16));
    w.slab = reinterpret_cast<uint32_t*>(take(static_cast<uint64_t>(select_flag_blocks(n, bins)) * bins * 4));
    if (select) {
        w.want = take(bins);
        w.block_sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(n)));
        w.idx_off = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
        w.dst_off = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
        w.klen = reinterpret_cast<uint32_t*>(take(n * 4));
        w.flags = take(n);
    }
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t select_workspace_bytes(uint64_t n, uint32_t K, bool select) { return select_workspace(nullptr, n, K, select).bytes; }

namespace {
template <typename OFF, bool SELECT>
void launch_flags_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n,
                     const void* off, const SelectWs& w, uint32_t lds_bins) {
    const OFF* o = static_cast<const OFF*>(off);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_select_flags<OFF, ROWS_U8, SELECT>), dim3(blocks), dim3(256), lds, stream, ids, row_units, K, n, o, w.want, w.flags, w.klen, w.slab,
                           w.counts, lds_bins, w.status);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_select_flags<OFF, ROWS_U16, SELECT>), dim3(blocks), dim3(256), lds, stream, ids, row_units, K, n, o, w.want, w.flags, w.klen, w.slab,
                           w.counts, lds_bins, w.status);
    else
        hipLaunchKernelGGL((k_select_flags<OFF, ROWS_DENSE, SELECT>), dim3(blocks), dim3(256), lds, stream, ids, row_units, K, n, o, w.want, w.flags, w.klen,
                           w.slab, w.counts, lds_bins, w.status);
}
}  // namespace

// The two scans behind a flags pass (k_select_flags, or gx_where.hip's k_where_flags) on the same stream: w.idx_off[0..n] from w.flags,
// w.dst_off[0..n] from w.klen.
hipError_t launch_select_scans(uint64_t n, const SelectWs& w, hipStream_t stream) {
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(w.idx_off, 0, 8, stream);
        return e != hipSuccess ? e : hipMemsetAsync(w.dst_off, 0, 8, stream);
    }
    const hipError_t e = launch_exclusive_scan<uint8_t>(w.flags, n, w.block_sums, w.idx_off, stream);
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.klen, n, w.block_sums, w.dst_off, stream);
}

// The flags pass.  offsets == nullptr: the histogram alone (w.counts[2K + 2]); else w.want holds the mask, and the pass and the two
// scans behind it leave w.flags, w.idx_off[0..n], w.dst_off[0..n] and w.status (1: a line of 4 G code units or more).
hipError_t launch_select_flags(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64,
                               const SelectWs& w, hipStream_t stream) {
    const uint32_t bins = 2u * K + 2u;
    const bool select = offsets != nullptr;
    hipError_t e = hipMemsetAsync(w.counts, 0, static_cast<size_t>(bins) * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(w.status, 0, 16, stream);
    if (e == hipSuccess && select && n == 0) e = launch_select_scans(0, w, stream);
    if (e != hipSuccess || n == 0) return e;
    const uint32_t lds_bins = bins <= SELECT_LDS_BINS ? bins : 0u;
    const uint32_t lds = lds_bins ? lds_bins * 4u + static_cast<uint32_t>(pad16(bins)) : 0u;
    const unsigned blocks = select_flag_blocks(n, bins);
    if (!select) launch_flags_as<uint32_t, false>(fmt, blocks, lds, stream, ids, row_units, K, n, nullptr, w, lds_bins);
    else if (offsets64) launch_flags_as<uint64_t, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, w, lds_bins);
    else launch_flags_as<uint32_t, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, w, lds_bins);
    if (lds_bins) hipLaunchKernelGGL(k_select_sum, dim3(bins), dim3(256), 0, stream, w.slab, blocks, bins, w.counts);
    e = hipGetLastError();
    if (e != hipSuccess || !select) return e;
    return launch_select_scans(n, w, stream);
}

// The copy pass, behind launch_select_flags on the same stream (and behind the host's look at the two totals: the outputs are as
// large as those say).
hipError_t launch_select_copy(const SelectOut& o, const void* data, const void* offsets, int offsets64, int wide, uint64_t n, const SelectWs& w,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    SelectCopy a{};
    a.src = static_cast<const uint8_t*>(data);
    a.unit_shift = wide ? 1u : 0u;
    a.n = n;
    a.flags = w.flags;
    a.idx_off = w.idx_off;
    a.dst_off = w.dst_off;
    a.out_index = o.index;
    a.out_bytes = static_cast<uint8_t*>(o.bytes);
    a.out_offsets = o.offsets;
    for (int q = 0; q < 2; ++q) a.col[q] = SelectColumn{o.col_src[q], o.col_dst[q], o.col_width[q], o.col_unit_bytes[q]};
    if (!a.col[0].src) { a.col[0] = a.col[1]; a.col[1] = SelectColumn{}; }
    const uint64_t tiles = (n + 63) >> 6;
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((tiles + 3) / 4, 256u * 16u));
    if (offsets64) hipLaunchKernelGGL(k_select_copy<uint64_t>, dim3(blocks), dim3(256), 0, stream, a, static_cast<const uint64_t*>(offsets));
    else hipLaunchKernelGGL(k_select_copy<uint32_t>, dim3(blocks), dim3(256), 0, stream, a, static_cast<const uint32_t*>(offsets));
    return hipGetLastError();
}

}  // namespace gx
