// gx_group_quantile.hip -- the passes of gx_group_quantiles / gx_text_group_quantiles behind gx_group_lines' own (gx_group.hip):
// percentiles of a captured number per captured text, on the device.  The rule -- the digit plan, the bounds, the pick -- is
// gx_group_quantile.hpp; DESIGN.md section 5.4.
//
// Before the host's ONE read of the totals (launch_gq_collect, behind launch_group_build on the same stream):
//   keys     gx_top_lines' k_top_keys itself (launch_top_keys) on the parts that have a value group: the class of every line's value,
//            a number's order-preserving key, the candidate flag.
//   flags    a candidate must also have a key: cand[i] &= slot_of[i] != GROUP_NONE (slot_of: the build pass's).
//   compact  ONE scan (gx_scan.hpp) of the 1-byte flags; k_gq_compact writes the candidates' (value key, slot) pairs densely, in line
//            order, and leaves every workgroup's OR and AND of its value keys; k_gq_masks, one workgroup, joins them in a fixed order.
//            OR and AND do not depend on any order in the first place.  The host reads them, and the number of candidates, in the wait
//            in which it reads the totals: the call has ONE wait before its outputs, as gx_group_lines has (host outputs: a second one
//            delivers them).
// Behind it and behind launch_group_emit, which numbers the slots' keys (launch_gq_sort_pick):
//   number   the pairs' slots become key numbers (k_gq_number).
//   sort     per digit of the host's plan: count (a workgroup owns GQ_BLOCK consecutive pairs and leaves its 64 counts), a scan of the
//            counts bin-major, scatter (every pair to the base of its bin + its rank among the pairs before it).  The ranks come from
//            ballots (gx_radix_dev.hpp, gx_partition.hip's scheme), never from atomics: the sort is stable whatever the waves' timing.
//   pick     one lane per (key, quantile): the key's run by binary search over the sorted key numbers, the rank, the value, and the
//            two bounds inside the run (gq_pick).
// No atomics in global memory, no workgroup waits for another, every loop is bounded by an argument or a constant.
//
// The workspace, per line of the batch: 8 (keys, later the second value buffer) + 8 (the scan) + 8 (the first value buffer) + 2 x 4 (the
// key-number buffers; the second holds the slots first) + 1 (the flags) = 33 bytes, and 12 bytes per GQ_BLOCK lines of counts and bases.
//
// -DGX_GQ_ALL_DIGITS (build.py --variant) is the other arm of the measurement in profiles/group_quantiles.txt: every value digit is
// sorted, whether two candidates differ in it or not.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_quantile.hpp"
#include "gx_radix_dev.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace {

constexpr uint32_t GQ_TILES = 8;                      // 64-pair tiles a wave owns in the sort's passes
constexpr uint32_t GQ_BLOCK = 4u * GQ_TILES * 64u;    // pairs a sort workgroup (four waves) owns: 2 048
constexpr uint32_t GQ_COMPACT_BLOCKS = 2048;

__global__ void __launch_bounds__(256) k_gq_flags(uint64_t n, const uint32_t* __restrict__ slot_of, uint8_t* __restrict__ cand) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride)
        if (cand[i] && slot_of[i] == GROUP_NONE) cand[i] = 0;
}

// vkey[at], slot[at] = line i's, at = the candidates before line i; masks[2 b], masks[2 b + 1] = workgroup b's OR and AND
__global__ void __launch_bounds__(256) k_gq_compact(const uint8_t* __restrict__ cand, const uint64_t* __restrict__ before, const uint64_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ slot_of, uint64_t n, uint64_t* __restrict__ vkey, uint32_t* __restrict__ slot,
                                                    uint64_t* __restrict__ masks) {
    __shared__ uint64_t w_or[4], w_and[4];
    uint64_t o = 0ull, a = ~0ull;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!cand[i]) continue;
        const uint64_t at = before[i], k = keys[i];
        o |= k;
        a &= k;
        if (at < n) {   // (it is: at most i candidates lie before line i)
            vkey[at] = k;
            slot[at] = slot_of[i];
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        o |= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(o), d));
        a &= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(a), d));
    }
    if ((threadIdx.x & 63u) == 0u) { w_or[threadIdx.x >> 6] = o; w_and[threadIdx.x >> 6] = a; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        masks[2u * blockIdx.x] = w_or[0] | w_or[1] | w_or[2] | w_or[3];
        masks[2u * blockIdx.x + 1u] = w_and[0] & w_and[1] & w_and[2] & w_and[3];
    }
}

__global__ void __launch_bounds__(256) k_gq_masks(const uint64_t* __restrict__ masks, uint32_t blocks, const uint64_t* __restrict__ total, GqDev* __restrict__ head) {
    __shared__ uint64_t w_or[4], w_and[4];
    uint64_t o = 0ull, a = ~0ull;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) { o |= masks[2u * b]; a &= masks[2u * b + 1u]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        o |= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(o), d));
        a &= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(a), d));
    }
    if ((threadIdx.x & 63u) == 0u) { w_or[threadIdx.x >> 6] = o; w_and[threadIdx.x >> 6] = a; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        head->value_or = w_or[0] | w_or[1] | w_or[2] | w_or[3];
        head->value_and = w_and[0] & w_and[1] & w_and[2] & w_and[3];
        head->candidates = *total;
    }
}

// slot -> key number, behind the emit pass (keynum[] is written for every slot that holds a key)
__global__ void __launch_bounds__(256) k_gq_number(const uint32_t* __restrict__ slot, uint32_t m, const uint32_t* __restrict__ keynum, uint32_t n_slots,
                                                   uint32_t* __restrict__ knum) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < m; i += stride) {
        const uint32_t s = slot[i];
        knum[i] = s < n_slots ? keynum[s] : GROUP_NONE;   // (it is: a candidate has a slot)
    }
}

// slab[bin * gridDim.x + workgroup] = the workgroup's pairs whose digit is `bin` (k_part_count's layout)
template <typename WORD>
__global__ void __launch_bounds__(256) k_gq_count(const WORD* __restrict__ words, uint32_t m, uint32_t shift, uint32_t* __restrict__ slab) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * GQ_BLOCK + static_cast<uint64_t>(wave) * (GQ_TILES * 64u);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < GQ_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = valid ? gq_digit(words[i], shift) : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(digit, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) slab[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x] = wcnt[0][lane] + wcnt[1][lane] + wcnt[2][lane] + wcnt[3][lane];
}

// ON_KEY: the digit is the key number's, else the value key's.  Both words of a pair travel.
template <bool ON_KEY>
__global__ void __launch_bounds__(256) k_gq_scatter(const uint64_t* __restrict__ vin, const uint32_t* __restrict__ kin, uint32_t m, uint32_t shift,
                                                    const uint64_t* __restrict__ bases, uint64_t* __restrict__ vout, uint32_t* __restrict__ kout) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * GQ_BLOCK + static_cast<uint64_t>(wave) * (GQ_TILES * 64u);
    uint64_t v[GQ_TILES];
    uint32_t k[GQ_TILES];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < GQ_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        v[t] = valid ? vin[i] : 0ull;
        k[t] = valid ? kin[i] : 0u;
        const uint32_t digit = ON_KEY ? gq_digit(k[t], shift) : gq_digit(v[t], shift);
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(digit, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    // lane b: where bin b's next pair of this wave goes (m < 2^32)
    uint32_t next = static_cast<uint32_t>(bases[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x]);
    for (uint32_t w = 0; w < wave; ++w) next += wcnt[w][lane];
#pragma unroll
    for (uint32_t t = 0; t < GQ_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = ON_KEY ? gq_digit(k[t], shift) : gq_digit(v[t], shift);
        const DigitBallots b = digit_ballots(digit, valid);
        const uint64_t same = bin_mask(b, digit);
        const uint32_t rank = static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
        const uint32_t to = static_cast<uint32_t>(__shfl(static_cast<int>(next), static_cast<int>(digit))) + rank;
        next += static_cast<uint32_t>(__popcll(bin_mask(b, lane)));
        if (valid && to < m) {   // (it is: the bases and the ranks count these very m pairs)
            vout[to] = v[t];
            kout[to] = k[t];
        }
    }
}

// rows[j * n_q + q], j < n_keys: one lane each
__global__ void __launch_bounds__(256) k_gq_pick(const uint32_t* __restrict__ knum, const uint64_t* __restrict__ vkey, uint32_t m, const QuantHead* __restrict__ asks,
                                                 uint32_t n_q, uint64_t n_keys, QuantOut* __restrict__ rows) {
    const uint64_t at = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (at >= n_keys * n_q) return;
    const uint32_t j = static_cast<uint32_t>(at / n_q), q = static_cast<uint32_t>(at - static_cast<uint64_t>(j) * n_q);
    rows[at] = gq_pick(knum, vkey, m, j, asks->ask[q].num, asks->ask[q].den);
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint64_t gq_blocks(uint64_t m) { return (m + GQ_BLOCK - 1) / GQ_BLOCK; }
uint32_t line_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, GQ_COMPACT_BLOCKS)); }

}  // namespace

GqWs gq_workspace(void* ws, uint64_t n) {
    const uint64_t slab = GQ_BINS * gq_blocks(n);
    GqWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.head = take(sizeof(GqDev));
    w.masks = reinterpret_cast<uint64_t*>(take(GQ_COMPACT_BLOCKS * 16u));
    w.slab = reinterpret_cast<uint32_t*>(take(std::max<uint64_t>(static_cast<uint64_t>(top_keys_blocks(n)) * TOP_COUNTS, slab) * 4));
    w.bases = reinterpret_cast<uint64_t*>(take((slab + 1) * 8));
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n), scan_sums_bytes(slab))));
    w.keys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.vkey[0] = reinterpret_cast<uint64_t*>(take(n * 8));
    w.vkey[1] = w.keys;   // (the per-line keys are read for the last time by the compaction, before the first pass of the sort)
    w.knum[0] = reinterpret_cast<uint32_t*>(take(n * 4));
    w.knum[1] = reinterpret_cast<uint32_t*>(take(n * 4));
    w.cand = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t gq_workspace_bytes(uint64_t n) { return gq_workspace(nullptr, n).bytes; }

bool gq_sorts_all_digits() {
#ifdef GX_GQ_ALL_DIGITS
    return true;
#else
    return false;
#endif
}

// Behind launch_group_build on `stream`; n > 0 and a.image names at least one part.  Leaves GqDev at w.head, and the candidates' value
// keys in w.vkey[0] and slots in w.knum[1], in line order.
hipError_t launch_gq_collect(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                             const uint32_t* slot_of, const GqWs& w, hipStream_t stream) {
    GqDev* head = reinterpret_cast<GqDev*>(w.head);
    hipError_t e = hipMemsetAsync(head, 0, sizeof(GqDev), stream);
    if (e != hipSuccess) return e;
    TopWs tw{};
    tw.keys = w.keys;
    tw.cand = w.cand;
    tw.slab = w.slab;
    e = launch_top_keys(ids, fmt, row_units, K, n, offsets, offsets64, a, tw, head->counts, stream);
    if (e != hipSuccess) return e;
    const unsigned lb = line_blocks(n);
    hipLaunchKernelGGL(k_gq_flags, dim3(lb), dim3(256), 0, stream, n, slot_of, w.cand);
    e = launch_exclusive_scan<uint8_t>(w.cand, n, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gq_compact, dim3(lb), dim3(256), 0, stream, w.cand, w.before, w.keys, slot_of, n, w.vkey[0], w.knum[1], w.masks);
    hipLaunchKernelGGL(k_gq_masks, dim3(1), dim3(256), 0, stream, w.masks, lb, w.before + n, head);
    return hipGetLastError();
}

// Behind launch_gq_collect, the host's read of GqDev and launch_group_emit on `stream`: m = the candidates (0 < m <= n), plan from
// gq_plan, n_keys * n_q rows at `rows`.
hipError_t launch_gq_sort_pick(const GqWs& w, uint64_t m, const GqPlan& plan, const uint32_t* keynum, uint32_t n_slots, const void* quant_head, uint32_t n_q,
                               uint64_t n_keys, void* rows, hipStream_t stream) {
    if (m == 0 || m > 0xFFFFFFFFull || n_q == 0 || n_q > QUANT_MAX || plan.n_passes > GQ_MAX_PASSES) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    const uint64_t blocks64 = gq_blocks(m);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    hipLaunchKernelGGL(k_gq_number, dim3(line_blocks(m)), dim3(256), 0, stream, w.knum[1], m32, keynum, n_slots, w.knum[0]);
    uint32_t cur = 0;
    for (uint32_t p = 0; p < plan.n_passes; ++p) {
        const uint32_t shift = plan.pass[p].shift;
        const bool on_key = plan.pass[p].on_key != 0;
        if (on_key) hipLaunchKernelGGL(k_gq_count<uint32_t>, dim3(blocks), dim3(256), 0, stream, w.knum[cur], m32, shift, w.slab);
        else hipLaunchKernelGGL(k_gq_count<uint64_t>, dim3(blocks), dim3(256), 0, stream, w.vkey[cur], m32, shift, w.slab);
        const hipError_t e = launch_exclusive_scan<uint32_t>(w.slab, GQ_BINS * blocks64, w.block_sums, w.bases, stream);
        if (e != hipSuccess) return e;
        if (on_key) hipLaunchKernelGGL(k_gq_scatter<true>, dim3(blocks), dim3(256), 0, stream, w.vkey[cur], w.knum[cur], m32, shift, w.bases, w.vkey[cur ^ 1u], w.knum[cur ^ 1u]);
        else hipLaunchKernelGGL(k_gq_scatter<false>, dim3(blocks), dim3(256), 0, stream, w.vkey[cur], w.knum[cur], m32, shift, w.bases, w.vkey[cur ^ 1u], w.knum[cur ^ 1u]);
        cur ^= 1u;
    }
    // (cur == gq_result_buffer(plan))
    const uint64_t lanes = n_keys * n_q;
    if (lanes == 0) return hipGetLastError();
    hipLaunchKernelGGL(k_gq_pick, dim3(static_cast<unsigned>((lanes + 255) / 256)), dim3(256), 0, stream, w.knum[cur], w.vkey[cur], m32,
                       static_cast<const QuantHead*>(quant_head), n_q, n_keys, static_cast<QuantOut*>(rows));
    return hipGetLastError();
}

}  // namespace gx
