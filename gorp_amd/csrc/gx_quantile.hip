// gx_quantile.hip -- the passes of gx_capture_quantiles / gx_text_capture_quantiles: percentiles of a number the lines of a finished
// batch captured, on the device.  The reference's caller asks this of its results right behind the extraction (README.md:26,63-79:
// the median and the p95 / p99 of timeTakenInMsec).  The rule -- the rank, the select's state, the grouping, the pick -- is
// gx_quantile.hpp; DESIGN.md section 5.4.
//
//   keys     gx_top_lines' k_top_keys itself (launch_top_keys, gx_top.hip): the line's class, a number's key, the candidate flag, and
//            the summed class counts.
//   compact  ONE scan (gx_scan.hpp) of the 1-byte flags, and k_quant_compact writes the candidates' keys densely, in line order.  From
//            here on nothing reads a per-line column.
//   begin    one wave: the ranks and the first state from the summed count of numbers.
//   select   eight digits, most significant first, two launches each.  k_quant_hist sweeps the dense keys, several per lane and trip with
//            the loads issued together; a 256-bin LDS histogram per group; a slab per workgroup.  k_quant_pick, one workgroup per quantile
//            and one lane per bin, sums its group's slabs, makes the suffix sums in LDS, and the one lane whose bin is picked applies
//            quant_step; behind digit 0 that lane writes the quantile's result row.
//
// Both kernels of a digit work the digit's grouping out for themselves from the 16 states (quant_rep: at most 16 x 16 compares), instead
// of the pick leaving it for the next sweep: a pick's workgroups, one per quantile, cannot see each other's picks within a launch
// without waiting for one another.  For the same reason the state is kept twice (QuantDev).
//
// No atomics in global memory, no workgroup waits for another, every loop is bounded by an argument or a constant: every output has
// the same bits on every run.
//
// -DGX_QUANT_NO_COMPACT (build.py --variant) is the other arm of the measurement in profiles/capture_quantiles.txt: no scan, no dense
// list; the sweeps read the flag and then the key of every line as k_top_hist does.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_quantile.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace {

constexpr uint32_t SWEEP_KEYS = 4;       // keys a lane of a sweep takes per trip
constexpr uint32_t SWEEP_BLOCKS = 512;   // workgroups of a sweep at most: a pick adds up that many slabs per bin
constexpr uint32_t PICK_THREADS = 1024;  // four lanes per bin add the slabs up

// ckeys[0 .. numbers) = the candidates' keys in line order
__global__ void __launch_bounds__(256) k_quant_compact(const uint8_t* __restrict__ cand, const uint64_t* __restrict__ before, const uint64_t* __restrict__ keys,
                                                       uint64_t n, uint64_t* __restrict__ ckeys) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!cand[i]) continue;
        const uint64_t at = before[i];
        if (at < n) ckeys[at] = keys[i];   // (it is: at most i candidates lie before line i)
    }
}

__global__ void __launch_bounds__(64) k_quant_begin(QuantDev* __restrict__ head, const QuantHead* __restrict__ asks) {
    const uint32_t q = threadIdx.x;
    if (q < asks->n_q && q < QUANT_MAX) quant_begin(head->sel[(TOP_DIGITS - 1u) & 1u][q], asks->ask[q].num, asks->ask[q].den, head->counts[TOP_C_NUMBERS]);
}

// The grouping before digit d, by the first QUANT_MAX lanes of a workgroup into LDS (the caller synchronises behind it).
struct GroupsLds {
    uint8_t rep[QUANT_MAX], group_of[QUANT_MAX];
    uint64_t prefix[QUANT_MAX];   // group -> its representative's prefix
    uint32_t n_groups;
};
__device__ void groups_to_lds(const QuantSelect* __restrict__ sel, uint32_t n_q, uint32_t d, GroupsLds& g) {
    const uint32_t q = threadIdx.x;
    if (q < n_q) g.rep[q] = static_cast<uint8_t>(quant_rep(sel, q, d));
    __syncthreads();
    if (q < n_q) {
        const uint32_t at = quant_group_of(g.rep, q);
        g.group_of[q] = static_cast<uint8_t>(at);
        if (g.rep[q] == q) g.prefix[at] = sel[q].prefix;
    }
    if (q == 0u) g.n_groups = quant_group_count(g.rep, n_q);
}

// slab[blockIdx.x][group][256]: by digit d, the keys under every group's prefix.  COMPACT: `keys` is the dense list and the head's
// count of numbers its length (n: the lines, an upper bound the grid was sized by); else keys and cand are per line.  A wave takes
// SWEEP_KEYS x 64 consecutive keys a trip, loaded together.  A key lies under at most one group's prefix -- the groups' prefixes differ
// above d -- so it is compared with each live group's and counted once, in LDS.  A wave whose counted lanes all hold the same group
// and digit -- small numbers share every high digit -- adds once; else every lane adds for itself.
template <bool COMPACT>
__global__ void __launch_bounds__(256) k_quant_hist(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cand, uint64_t n,
                                                    const QuantDev* __restrict__ head, uint32_t n_q, uint32_t d, uint32_t* __restrict__ slab) {
    __shared__ uint32_t h[QUANT_MAX * TOP_BINS];
    __shared__ GroupsLds g;
    const uint64_t numbers = head->counts[TOP_C_NUMBERS];
    const uint64_t count = COMPACT ? (numbers < n ? numbers : n) : n;
    groups_to_lds(head->sel[d & 1u], n_q, d, g);
    __syncthreads();
    const uint32_t n_groups = g.n_groups;   // 1 .. n_q
    for (uint32_t j = threadIdx.x; j < n_groups * TOP_BINS; j += 256u) h[j] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u * SWEEP_KEYS;
    if (numbers != 0u) {
        for (uint64_t i0 = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)) * SWEEP_KEYS; i0 < count; i0 += stride) {
            bool c[SWEEP_KEYS];
            uint64_t key[SWEEP_KEYS];
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_KEYS; ++u) {
                const uint64_t i = i0 + u * 64u + lane;
                c[u] = i < count && (COMPACT || cand[i] != 0);
            }
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_KEYS; ++u) key[u] = c[u] ? keys[i0 + u * 64u + lane] : 0ull;
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_KEYS; ++u) {
                uint32_t at = n_groups;
                for (uint32_t j = 0; j < n_groups; ++j)
                    if (top_in_prefix(key[u], g.prefix[j], d)) at = j;
                const bool counted = c[u] && at < n_groups;
                const uint32_t code = at * TOP_BINS + top_digit(key[u], d);
                const uint64_t m = __ballot(counted);
                if (m != 0ull) {   // (the same in every lane of the wave)
                    const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(m))) - 1u;
                    const uint32_t wc = static_cast<uint32_t>(__shfl(static_cast<int>(code), static_cast<int>(l)));
                    if (__ballot(counted && code == wc) == m) {
                        if (lane == l) atomicAdd(&h[wc], static_cast<uint32_t>(__popcll(m)));
                    } else if (counted) {
                        atomicAdd(&h[code], 1u);   // (code < n_groups * 256)
                    }
                }
            }
        }
    }
    __syncthreads();
    uint32_t* mine = slab + static_cast<uint64_t>(blockIdx.x) * n_groups * TOP_BINS;
    for (uint32_t j = threadIdx.x; j < n_groups * TOP_BINS; j += 256u) mine[j] = h[j];
}

// One workgroup per quantile: digit d's step on its state.  Lane t adds up bin t & 255 of every fourth slab of the quantile's group, in
// the slabs' order; the four partial sums meet in LDS, a suffix scan over the 256 bins gives S(b), and the one lane with
// S(b) >= remaining > S(b + 1) applies the step.  Behind digit 0 it writes the result row.
__global__ void __launch_bounds__(PICK_THREADS) k_quant_pick(QuantDev* __restrict__ head, uint32_t n_q, uint32_t d, const uint32_t* __restrict__ slab,
                                                             uint32_t blocks) {
    __shared__ GroupsLds g;
    __shared__ uint32_t part[PICK_THREADS / TOP_BINS][TOP_BINS];
    __shared__ uint32_t S[2][TOP_BINS + 1];
    const QuantSelect* sel = head->sel[d & 1u];
    groups_to_lds(sel, n_q, d, g);
    __syncthreads();
    const uint32_t q = blockIdx.x;   // < n_q
    const uint32_t n_groups = g.n_groups, mine = g.group_of[q];
    const uint32_t bin = threadIdx.x & (TOP_BINS - 1u), slice = threadIdx.x / TOP_BINS;
    uint32_t t = 0;   // (every count is below 2^32: so is the number of lines)
#pragma unroll 8
    for (uint32_t b = slice; b < blocks; b += PICK_THREADS / TOP_BINS) t += slab[(static_cast<uint64_t>(b) * n_groups + mine) * TOP_BINS + bin];
    part[slice][bin] = t;
    __syncthreads();
    uint32_t cur = 0;
    if (threadIdx.x < TOP_BINS) S[0][bin] = part[0][bin] + part[1][bin] + part[2][bin] + part[3][bin];
    if (threadIdx.x == TOP_BINS) S[0][TOP_BINS] = S[1][TOP_BINS] = 0u;
    __syncthreads();
    for (uint32_t step = 1; step < TOP_BINS; step <<= 1) {   // S[cur][b] = the sum of the bins b .. min(b + step, 256) - 1
        if (threadIdx.x < TOP_BINS) S[cur ^ 1u][bin] = S[cur][bin] + (bin + step < TOP_BINS ? S[cur][bin + step] : 0u);
        cur ^= 1u;
        __syncthreads();
    }
    if (threadIdx.x < TOP_BINS) {
        const QuantSelect was = sel[q];
        const uint64_t s_b = S[cur][bin], s_b1 = S[cur][bin + 1u];
        if (was.rank != 0u && quant_picked(s_b, s_b1, was.remaining)) {
            QuantSelect now = was;
            quant_step(now, quant_pick_of(bin, s_b1, was.remaining), static_cast<uint32_t>(s_b - s_b1), d);
            head->sel[(d & 1u) ^ 1u][q] = now;
            if (d == 0u) head->out[q] = quant_out(now, head->counts[TOP_C_NUMBERS]);
        }
    }
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint32_t sweep_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 256u * SWEEP_KEYS - 1) / (256u * SWEEP_KEYS), SWEEP_BLOCKS)); }
uint32_t compact_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, 2048)); }

}  // namespace

QuantWs quant_workspace(void* ws, uint64_t n) {
    QuantWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.head = take(sizeof(QuantDev));
    w.slab = reinterpret_cast<uint32_t*>(take(std::max<uint64_t>(static_cast<uint64_t>(top_keys_blocks(n)) * TOP_COUNTS,
                                                                 static_cast<uint64_t>(sweep_blocks(n)) * QUANT_MAX * TOP_BINS) * 4));
    w.block_sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(n)));
    w.keys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.ckeys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.cand = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t quant_workspace_bytes(uint64_t n) { return quant_workspace(nullptr, n).bytes; }

hipError_t launch_quantiles(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                            const void* quant_head, uint32_t n_quantiles, const QuantWs& w, hipStream_t stream) {
    if (n_quantiles > QUANT_MAX) return hipErrorInvalidValue;
    QuantDev* head = reinterpret_cast<QuantDev*>(w.head);
    hipError_t e = hipMemsetAsync(head, 0, sizeof(QuantDev), stream);
    if (e != hipSuccess) return e;
    TopWs tw{};
    tw.keys = w.keys;
    tw.cand = w.cand;
    tw.slab = w.slab;
    e = launch_top_keys(ids, fmt, row_units, K, n, offsets, offsets64, a, tw, head->counts, stream);
    if (e != hipSuccess || n_quantiles == 0u) return e;
#ifndef GX_QUANT_NO_COMPACT
    e = launch_exclusive_scan<uint8_t>(w.cand, n, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_quant_compact, dim3(compact_blocks(n)), dim3(256), 0, stream, w.cand, w.before, w.keys, n, w.ckeys);
#endif
    hipLaunchKernelGGL(k_quant_begin, dim3(1), dim3(64), 0, stream, head, static_cast<const QuantHead*>(quant_head));
    const unsigned sb = sweep_blocks(n);
    for (uint32_t d = TOP_DIGITS; d-- > 0u;) {
#ifndef GX_QUANT_NO_COMPACT
        hipLaunchKernelGGL(k_quant_hist<true>, dim3(sb), dim3(256), 0, stream, w.ckeys, static_cast<const uint8_t*>(nullptr), n, head, n_quantiles, d, w.slab);
#else
        hipLaunchKernelGGL(k_quant_hist<false>, dim3(sb), dim3(256), 0, stream, w.keys, w.cand, n, head, n_quantiles, d, w.slab);
#endif
        hipLaunchKernelGGL(k_quant_pick, dim3(n_quantiles), dim3(PICK_THREADS), 0, stream, head, n_quantiles, d, w.slab, sb);
    }
    return hipGetLastError();
}

}  // namespace gx
