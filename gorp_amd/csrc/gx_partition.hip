// gx_partition.hip -- the lines of a finished batch ordered by (outcome index, input line number): every sink's lines at once
// (gx_partition_lines).  One call per extraction of gx_select_lines costs a flags pass, two scans and a synchronisation each and
// reads the id column K times; a stable partition reads it once.
//
// Keys (k_part_keys): one read of the ids and the offsets; key = the outcome index (gx_outcome.hpp) if it is wanted, else
// 2K + 1 -- the largest key, so everything that is not kept sorts behind everything that is -- and the line's length, 0 if not
// kept.  Sort: a stable LSD radix sort of the line numbers by key, six bits a digit -- 64 bins, one per lane of a wave.  Per
// digit: count (k_part_count: a workgroup owns PART_BLOCK consecutive lines and leaves its 64 counts), a scan of the counts
// bin-major (gx_scan.hpp), scatter (k_part_scatter: every line to base of its bin + its rank among the lines before it).  The
// ranks come from ballots, not from atomics: the order of the output is the order of the input, whatever the waves' timing.
// The last digit's scatter also leaves the sorted keys and the permuted lengths; their scan gives the destination offsets, and
// k_part_groups the boundaries of the groups -- by binary search over the sorted keys: no histogram is needed -- for the host's
// one read.  Copy (k_part_copy): after a partition neighbours in the output are no neighbours in the input, so there are no
// runs to copy; the pass is built by DESTINATION chunk: a wave owns 64 consecutive output lines -- one contiguous span of the
// output -- and every lane writes one aligned 16-byte chunk of it per step, from two aligned 16-byte loads of its line's
// source joined by v_alignbyte.  DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_outcome.hpp"
#include "gx_radix_dev.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace {

constexpr uint32_t PART_TILES = 8;                        // 64-line tiles a wave owns in the sort's passes
constexpr uint32_t PART_BLOCK = 4u * PART_TILES * 64u;    // lines a sort workgroup (four waves) owns: 2 048

template <typename OFF, RowFormat F>
__global__ void __launch_bounds__(256) k_part_keys(const void* __restrict__ ids, uint32_t row_units, uint32_t K, uint64_t n, const OFF* __restrict__ off,
                                                   const uint8_t* __restrict__ want, uint32_t* __restrict__ keys, uint32_t* __restrict__ klen,
                                                   uint32_t* __restrict__ status) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
        const bool kept = oc <= 2u * K && want[oc] != 0;
        const uint64_t len = static_cast<uint64_t>(off[i + 1]) - static_cast<uint64_t>(off[i]);
        if (len > 0xFFFFFFFFull) atomicOr(status, 1u);   // (a line of 4 G code units: refused by the host)
        keys[i] = kept ? oc : 2u * K + 1u;
        klen[i] = kept ? static_cast<uint32_t>(len) : 0u;
    }
}

// slab[bin * gridDim.x + workgroup] = the workgroup's lines whose digit is `bin`
__global__ void __launch_bounds__(256) k_part_count(const uint32_t* __restrict__ keys, uint64_t n, uint32_t shift, uint32_t* __restrict__ slab) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * PART_BLOCK + static_cast<uint64_t>(wave) * (PART_TILES * 64u);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < PART_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < n;
        const uint32_t digit = valid ? (keys[i] >> shift) & 63u : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(digit, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) slab[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x] = wcnt[0][lane] + wcnt[1][lane] + wcnt[2][lane] + wcnt[3][lane];
}

// FIRST: the value that travels is the line's own number (there is no permutation yet).  LAST: the permuted lengths leave too.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) k_part_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, uint64_t n, uint32_t shift,
                                                      const uint64_t* __restrict__ bases, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ perm_out,
                                                      const uint32_t* __restrict__ klen, uint32_t* __restrict__ plen) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * PART_BLOCK + static_cast<uint64_t>(wave) * (PART_TILES * 64u);
    uint32_t key[PART_TILES];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < PART_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < n;
        key[t] = valid ? keys[i] : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots((key[t] >> shift) & 63u, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    // lane b: where bin b's next line of this wave goes (n < 2^32)
    uint32_t next = static_cast<uint32_t>(bases[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x]);
    for (uint32_t w = 0; w < wave; ++w) next += wcnt[w][lane];
#pragma unroll
    for (uint32_t t = 0; t < PART_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < n;
        const uint32_t digit = (key[t] >> shift) & 63u;
        const DigitBallots b = digit_ballots(digit, valid);
        const uint64_t same = bin_mask(b, digit);
        const uint32_t rank = static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
        const uint32_t to = static_cast<uint32_t>(__shfl(static_cast<int>(next), static_cast<int>(digit))) + rank;
        next += static_cast<uint32_t>(__popcll(bin_mask(b, lane)));
        if (valid) {
            const uint32_t v = FIRST ? static_cast<uint32_t>(i) : perm[i];
            keys_out[to] = key[t];
            perm_out[to] = v;
            if (LAST) plen[to] = klen[v];
        }
    }
}

// The boundaries of the groups, a lane per boundary: g[x] = lines with a key below x (x = 0 .. 2K + 1), g[2K + 2] = g[2K + 1] -- the
// kept lines; bin 2K + 1 is an empty group -- and u[x] = dst_off[g[x]], the same in code units.
__global__ void __launch_bounds__(256) k_part_groups(const uint32_t* __restrict__ sorted_keys, uint64_t n, uint32_t K, const uint64_t* __restrict__ dst_off,
                                                     uint64_t* __restrict__ g, uint64_t* __restrict__ u) {
    const uint32_t top = 2u * K + 1u;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x <= top + 1u) {
        const uint32_t k = x < top ? x : top;
        uint64_t lo = 0, hi = n;   // first line whose key is >= k
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (sorted_keys[mid] >= k) hi = mid;
            else lo = mid + 1;
        }
        g[x] = lo;
        u[x] = dst_off[lo];
    }
}

struct PartColumn {
    const void* src;
    void* dst;
    uint32_t width;       // units per line
    uint32_t unit_bytes;  // 1, 2 or 4
};

struct PartCopy {
    const uint8_t* src;        // the batch's code units
    uint32_t unit_shift;       // 0: bytes, 1: UTF-16 code units
    uint64_t n;                // lines of the input
    uint64_t kept;             // lines of the output
    const uint32_t* perm;      // [kept] the input line of output line j
    const uint64_t* dst_off;   // [kept + 1] code units before output line j
    uint32_t* out_index;       // optional
    uint8_t* out_bytes;        // optional
    void* out_offsets;         // optional, OFF[kept + 1]
    PartColumn col[2];         // src == nullptr: none
};

// A fixed-size column of the tile's `lines` output lines, the wave's lanes on consecutive units of the destination.
template <typename UNIT>
__device__ __forceinline__ void gather_column(const PartColumn& c, uint64_t j0, uint32_t lines, const uint32_t* tile_perm, uint32_t lane) {
    const UNIT* s = static_cast<const UNIT*>(c.src);
    UNIT* d = static_cast<UNIT*>(c.dst) + j0 * c.width;
    const uint32_t total = lines * c.width;
    for (uint32_t t = lane; t < total; t += 64u) {
        const uint32_t j = t / c.width, q = t - j * c.width;
        d[t] = s[static_cast<uint64_t>(tile_perm[j]) * c.width + q];
    }
}

template <typename OFF>
__global__ void __launch_bounds__(256) k_part_copy(PartCopy a, const OFF* __restrict__ off) {
    // per wave, per line of its tile: where the line ends in the output (an address), source address minus destination address,
    // and the input line
    __shared__ uint64_t ends[4][64];
    __shared__ uint64_t delta[4][64];
    __shared__ uint32_t perms[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t* end = ends[wave];
    uint64_t* dlt = delta[wave];
    uint32_t* tile_perm = perms[wave];
    const uint64_t kept = a.kept, tiles = (kept + 63u) >> 6;
    const uint32_t sh = a.unit_shift;
    const uintptr_t src0 = reinterpret_cast<uintptr_t>(a.src), out0 = reinterpret_cast<uintptr_t>(a.out_bytes);
    const uintptr_t lo = src0 + (static_cast<uint64_t>(off[0]) << sh), hi = src0 + (static_cast<uint64_t>(off[a.n]) << sh);
    OFF* out_off = static_cast<OFF*>(a.out_offsets);
    if (out_off && blockIdx.x == 0 && threadIdx.x == 0) out_off[kept] = static_cast<OFF>(a.dst_off[kept]);
    for (uint64_t tile = static_cast<uint64_t>(blockIdx.x) * 4u + wave; tile < tiles; tile += static_cast<uint64_t>(gridDim.x) * 4u) {
        const uint64_t j0 = tile << 6, j = j0 + lane;
        const uint32_t lines = static_cast<uint32_t>(kept - j0 < 64u ? kept - j0 : 64u);
        const bool valid = lane < lines;
        const uint64_t jj = valid ? j : kept - 1u;
        const uint32_t p = a.perm[jj];
        const uint64_t d0 = a.dst_off[jj], d1 = a.dst_off[jj + 1u];
        if (valid) {
            if (a.out_index) a.out_index[j] = p;
            if (out_off) out_off[j] = static_cast<OFF>(d0);
        }
        if (!a.out_bytes && !a.col[0].src) continue;
        const uint64_t s0 = static_cast<uint64_t>(off[p]);
        // (lanes behind the tile's last line: an empty line at the span's end)
        end[lane] = out0 + (d1 << sh);
        dlt[lane] = (src0 + (s0 << sh)) - (out0 + (d0 << sh));
        tile_perm[lane] = p;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (a.out_bytes) {
            const uint64_t A0 = out0 + (static_cast<uint64_t>(__shfl(static_cast<unsigned long long>(d0), 0)) << sh);
            const uint64_t A1 = static_cast<uint64_t>(__shfl(static_cast<unsigned long long>(end[lane]), 63));
            for (uint64_t ca = (A0 & ~static_cast<uint64_t>(15)) + (static_cast<uint64_t>(lane) << 4); ca < A1; ca += 1024u) {
                const uint64_t from = ca < A0 ? A0 : ca, to = ca + 16u > A1 ? A1 : ca + 16u;
                // the line that holds byte `from`: the first one that ends behind it
                uint32_t l = 0;
#pragma unroll
                for (uint32_t step = 32; step >= 1; step >>= 1)
                    if (end[l + step - 1u] <= from) l += step;
                if (to - from == 16u && end[l] >= to) {
                    // the chunk lies inside one line: two aligned loads of the source, joined
                    const uint64_t s = ca + dlt[l];
                    const uint32_t m = static_cast<uint32_t>(s & 15u), q = m >> 2, r = m & 3u;
                    const uint8_t* sa = reinterpret_cast<const uint8_t*>(s - m);
                    const uint4 x = load16_within(sa, lo, hi);
                    uint4 y = x;
                    if (m) y = load16_within(sa + 16, lo, hi);
                    // the five dwords from dword q on (a shift per lane: selects, not a branch), then the byte shift
                    const uint32_t w0 = (q & 2u) ? x.z : x.x, w1 = (q & 2u) ? x.w : x.y, w2 = (q & 2u) ? y.x : x.z, w3 = (q & 2u) ? y.y : x.w,
                                   w4 = (q & 2u) ? y.z : y.x, w5 = (q & 2u) ? y.w : y.y;
                    const uint32_t t0 = (q & 1u) ? w1 : w0, t1 = (q & 1u) ? w2 : w1, t2 = (q & 1u) ? w3 : w2, t3 = (q & 1u) ? w4 : w3,
                                   t4 = (q & 1u) ? w5 : w4;
                    *reinterpret_cast<uint4*>(ca) = make_uint4(ab(t1, t0, r), ab(t2, t1, r), ab(t3, t2, r), ab(t4, t3, r));
                } else {
                    // a line boundary inside the chunk, or the span's first or last chunk (a neighbouring wave owns the rest of
                    // it): byte by byte, nothing is read back to merge
                    for (uint64_t at = from; at < to; ++at) {
                        while (end[l] <= at) ++l;
                        *reinterpret_cast<uint8_t*>(at) = *reinterpret_cast<const uint8_t*>(at + dlt[l]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const PartColumn& c = a.col[q];
            if (!c.src) continue;
            if (c.unit_bytes == 4u) gather_column<uint32_t>(c, j0, lines, tile_perm, lane);
            else if (c.unit_bytes == 2u) gather_column<uint16_t>(c, j0, lines, tile_perm, lane);
            else gather_column<uint8_t>(c, j0, lines, tile_perm, lane);
        }
        // (the tables are rewritten by the wave's next tile)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void __launch_bounds__(256) k_part_pick(const uint64_t* __restrict__ from, const uint64_t* __restrict__ at, uint32_t count, uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) out[i] = from[at[i]];
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint64_t part_blocks(uint64_t n) { return (n + PART_BLOCK - 1) / PART_BLOCK; }

}  // namespace

uint32_t partition_digits(uint32_t K) {
    uint32_t bits = 1;
    while ((1ull << bits) < 2ull * K + 2ull) ++bits;
    return (bits + 5u) / 6u;
}

PartWs partition_workspace(void* ws, uint64_t n, uint32_t K) {
    const uint64_t bins = 2ull * K + 2ull, slab = 64u * part_blocks(n);
    PartWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.groups = reinterpret_cast<uint64_t*>(take((2 * (bins + 1) + 2) * 8));
    w.status = reinterpret_cast<uint32_t*>(w.groups + 2 * (bins + 1));
    w.want = take(bins);
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n), scan_sums_bytes(slab))));
    w.slab = reinterpret_cast<uint32_t*>(take(slab * 4));
    w.bases = reinterpret_cast<uint64_t*>(take((slab + 1) * 8));
    w.dst_off = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    for (int q = 0; q < 2; ++q) {
        w.keys[q] = reinterpret_cast<uint32_t*>(take(n * 4));
        w.perm[q] = reinterpret_cast<uint32_t*>(take(n * 4));
    }
    w.klen = reinterpret_cast<uint32_t*>(take(n * 4));
    w.plen = reinterpret_cast<uint32_t*>(take(n * 4));
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t partition_workspace_bytes(uint64_t n, uint32_t K) { return partition_workspace(nullptr, n, K).bytes; }

namespace {
template <typename OFF>
void launch_keys_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                    const PartWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_part_keys<OFF, ROWS_U8>), dim3(blocks), dim3(256), 0, stream, ids, row_units, K, n, o, w.want, w.keys[0], w.klen, w.status);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_part_keys<OFF, ROWS_U16>), dim3(blocks), dim3(256), 0, stream, ids, row_units, K, n, o, w.want, w.keys[0], w.klen, w.status);
    else
        hipLaunchKernelGGL((k_part_keys<OFF, ROWS_DENSE>), dim3(blocks), dim3(256), 0, stream, ids, row_units, K, n, o, w.want, w.keys[0], w.klen, w.status);
}
}  // namespace

// Keys, sort, scan and the groups, w.want holding the mask: leaves w.perm_sorted, w.dst_off[0 .. n], w.groups and w.status.
hipError_t launch_partition_sort(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, PartWs& w,
                                 hipStream_t stream) {
    const uint64_t bins = 2ull * K + 2ull;
    w.perm_sorted = w.perm[0];
    hipError_t e = hipMemsetAsync(w.groups, 0, (2 * (bins + 1) + 2) * 8, stream);   // (the status word behind them too)
    if (e != hipSuccess || n == 0) return e;
    const unsigned key_blocks = static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 256u * 16u));
    if (offsets64) launch_keys_as<uint64_t>(fmt, key_blocks, stream, ids, row_units, K, n, offsets, w);
    else launch_keys_as<uint32_t>(fmt, key_blocks, stream, ids, row_units, K, n, offsets, w);
    const uint64_t blocks64 = part_blocks(n);
    if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>(blocks64);
    const uint32_t digits = partition_digits(K);
    int cur = 0;
    for (uint32_t d = 0; d < digits; ++d) {
        const uint32_t shift = 6u * d;
        const bool first = d == 0, last = d + 1 == digits;
        const uint32_t *kin = w.keys[cur], *pin = w.perm[cur];
        uint32_t *kout = w.keys[cur ^ 1], *pout = w.perm[cur ^ 1];
        hipLaunchKernelGGL(k_part_count, dim3(blocks), dim3(256), 0, stream, kin, n, shift, w.slab);
        e = launch_exclusive_scan<uint32_t>(w.slab, 64u * blocks64, w.block_sums, w.bases, stream);
        if (e != hipSuccess) return e;
        if (first && last) hipLaunchKernelGGL((k_part_scatter<true, true>), dim3(blocks), dim3(256), 0, stream, kin, pin, n, shift, w.bases, kout, pout, w.klen, w.plen);
        else if (first) hipLaunchKernelGGL((k_part_scatter<true, false>), dim3(blocks), dim3(256), 0, stream, kin, pin, n, shift, w.bases, kout, pout, w.klen, w.plen);
        else if (last) hipLaunchKernelGGL((k_part_scatter<false, true>), dim3(blocks), dim3(256), 0, stream, kin, pin, n, shift, w.bases, kout, pout, w.klen, w.plen);
        else hipLaunchKernelGGL((k_part_scatter<false, false>), dim3(blocks), dim3(256), 0, stream, kin, pin, n, shift, w.bases, kout, pout, w.klen, w.plen);
        cur ^= 1;
    }
    w.perm_sorted = w.perm[cur];
    e = launch_exclusive_scan<uint32_t>(w.plen, n, w.block_sums, w.dst_off, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_part_groups, dim3(static_cast<unsigned>((bins + 1 + 255) / 256)), dim3(256), 0, stream, w.keys[cur], n, K, w.dst_off, w.groups, w.groups + bins + 1);
    return hipGetLastError();
}

// The copy pass, behind launch_partition_sort on the same stream and behind the host's look at the totals (`kept` lines; the
// outputs are as large as those say).
hipError_t launch_partition_copy(const SelectOut& o, const void* data, const void* offsets, int offsets64, int wide, uint64_t n, uint64_t kept, const PartWs& w,
                                 hipStream_t stream) {
    if (kept == 0) return hipSuccess;
    PartCopy a{};
    a.src = static_cast<const uint8_t*>(data);
    a.unit_shift = wide ? 1u : 0u;
    a.n = n;
    a.kept = kept;
    a.perm = w.perm_sorted;
    a.dst_off = w.dst_off;
    a.out_index = o.index;
    a.out_bytes = static_cast<uint8_t*>(o.bytes);
    a.out_offsets = o.offsets;
    for (int q = 0; q < 2; ++q) a.col[q] = PartColumn{o.col_src[q], o.col_dst[q], o.col_width[q], o.col_unit_bytes[q]};
    if (!a.col[0].src) { a.col[0] = a.col[1]; a.col[1] = PartColumn{}; }
    const uint64_t tiles = (kept + 63) >> 6;
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((tiles + 3) / 4, 256u * 64u));
    if (offsets64) hipLaunchKernelGGL(k_part_copy<uint64_t>, dim3(blocks), dim3(256), 0, stream, a, static_cast<const uint64_t*>(offsets));
    else hipLaunchKernelGGL(k_part_copy<uint32_t>, dim3(blocks), dim3(256), 0, stream, a, static_cast<const uint32_t*>(offsets));
    return hipGetLastError();
}

// out[i] = from[at[i]], i < count (gx_text_to_jsonl_by_extraction: where every group's JSON begins)
hipError_t launch_partition_pick(const uint64_t* from, const uint64_t* at, uint32_t count, uint64_t* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_part_pick, dim3((count + 255u) / 256u), dim3(256), 0, stream, from, at, count, out);
    return hipGetLastError();
}

}  // namespace gx
