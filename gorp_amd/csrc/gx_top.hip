// gx_top.hip -- the passes of gx_top_lines / gx_text_top_lines: the lines of a finished batch ranked by a number they captured, on
// the device.  The reference's caller does this behind the extraction (README.md:26,63-79): sorted(results, by timeTakenInMsec).take(N).
// The rule -- which lines are candidates, the key, the select step -- is gx_top.hpp; DESIGN.md section 5.4.
//
//   keys     one lane per line, grid-stride, the shape of k_capture_stats: the line's class, and for a number its key and a candidate
//            flag.  The class counts are ballot popcounts per wave, LDS adds per workgroup, a slab per workgroup and k_top_sum.
//   select   eight digits, most significant first: k_top_hist sweeps the key column and counts, by the digit, the candidates under the
//            prefix found so far (LDS histogram per workgroup, a slab, k_top_sum); the one-wave k_top_pick applies top_step to the
//            select's state in device memory.  The host reads nothing in between.
//   choose   k_top_flags marks key > T and key == T, ONE scan (gx_scan.hpp) counts both before every line -- the two counts share a
//            64-bit word -- and k_top_compact writes the chosen (key, line) pairs in line order: the ties taken are the earliest lines
//            whatever the waves' timing.
//   order    the chosen keys in every workgroup's LDS, a pair per lane: rank = keys above + equal keys at a lower index, visibly
//            stable.  Leaves the permutation, the values and the lines' lengths; a scan of the lengths gives the output offsets.
//   emit     launch_partition_copy (gx_partition.hip), called by gx_api.cpp behind the host's look at the totals.
//
// No atomics in global memory anywhere, so every output has the same bits on every run.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_outcome.hpp"
#include "gx_scan.hpp"
#include "gx_top.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t top_smem[];

constexpr uint32_t ORDER_THREADS = 256;
constexpr uint32_t SWEEP_LINES = 4;   // lines a lane of a sweep takes per trip
static_assert(TOP_MAX_LINES * 8u <= 64u * 1024u, "a workgroup of the order pass keeps every chosen key in LDS");

// LDS: the part image (TopHead), the term image (wimage_bytes, 0: no terms).  slab[blockIdx.x][TOP_COUNTS].
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_top_keys(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                  uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ timage,
                                                  const uint4* __restrict__ wimage, uint32_t wimage_bytes, uint64_t* __restrict__ keys,
                                                  uint8_t* __restrict__ cand, uint32_t* __restrict__ slab) {
    __shared__ uint32_t s_counts[TOP_COUNTS];
    uint8_t* smem = reinterpret_cast<uint8_t*>(top_smem);
    uint4* t_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(TopHead) >> 4); q += 256u) t_l[q] = timage[q];
    uint4* w_l = reinterpret_cast<uint4*>(smem + sizeof(TopHead));
    for (uint32_t q = threadIdx.x; q < (wimage_bytes >> 4); q += 256u) w_l[q] = wimage[q];
    if (threadIdx.x < TOP_COUNTS) s_counts[threadIdx.x] = 0u;
    __syncthreads();
    const TopHead* th = reinterpret_cast<const TopHead*>(smem);
    const WhereHead* wh = reinterpret_cast<const WhereHead*>(smem + sizeof(TopHead));
    const UNIT* lits = reinterpret_cast<const UNIT*>(smem + sizeof(TopHead) + sizeof(WhereHead));
    const uint32_t n_parts = th->n_parts;
    const bool smallest = th->smallest != 0u;
    const uint32_t ext_lo = th->ext[0], ext_hi = th->ext[n_parts - 1u];   // (n_parts > 0)
    const bool terms = wimage_bytes != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        uint32_t cls = 3u;   // 0: a number, 1: unset, 2: no number, 3: the line does not count
        bool too_long = false;
        if (i < n) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            const uint64_t o0 = static_cast<uint64_t>(off[i]);
            const uint64_t len = static_cast<uint64_t>(off[i + 1]) - o0;
            too_long = len > 0xFFFFFFFFull;                        // (a line of 4 G code units, or offsets that go backwards: refused by the host)
            const uint64_t line_units = too_long ? 0u : len;       // (no value is looked at in a line that is refused anyway)
            uint32_t e = n_parts;
            if (oc >= ext_lo && oc <= ext_hi) {                    // (oc <= ext_hi < K: a matched extraction)
                e = where_find(th->ext, n_parts, oc);
                if (e < n_parts && terms && !where_line_holds<F, UNIT, NUM>(wh, lits, oc, ids, caps, i, row_units, slots, data + o0, line_units)) e = n_parts;
            }
            if (e < n_parts) {
                int32_t pb, pe;
                int64_t v = 0;
                pair_of<F>(ids, caps, i, row_units, slots, th->group[e], pb, pe);
                if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                else cls = number_parse_packed<NUM>(NUM ? th->fmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                if (cls == 0u) keys[i] = top_key(v, smallest);
            }
            cand[i] = cls == 0u ? 1 : 0;
        }
        const uint64_t numbers = __ballot(cls == 0u), unset = __ballot(cls == 1u), not_numbers = __ballot(cls == 2u), longs = __ballot(too_long);
        if (lane == 0u) {
            if (numbers) atomicAdd(&s_counts[TOP_C_NUMBERS], static_cast<uint32_t>(__popcll(numbers)));
            if (unset) atomicAdd(&s_counts[TOP_C_UNSET], static_cast<uint32_t>(__popcll(unset)));
            if (not_numbers) atomicAdd(&s_counts[TOP_C_NOT_NUMBERS], static_cast<uint32_t>(__popcll(not_numbers)));
            if (longs) atomicAdd(&s_counts[TOP_C_STATUS], static_cast<uint32_t>(__popcll(longs)));
        }
    }
    __syncthreads();
    if (threadIdx.x < TOP_COUNTS) slab[static_cast<uint64_t>(blockIdx.x) * TOP_COUNTS + threadIdx.x] = s_counts[threadIdx.x];
}

// out[w] = the sum over the workgroups' slabs of word w, in a fixed order.  One workgroup per word.  (Every count is below 2^32: so
// is the number of lines.)
__global__ void __launch_bounds__(256) k_top_sum(const uint32_t* __restrict__ slab, uint32_t blocks, uint32_t total, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[4];
    const uint32_t w = blockIdx.x;
    uint32_t t = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) t += slab[static_cast<uint64_t>(b) * total + w];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[w] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(64) k_top_begin(TopDev* __restrict__ head, uint32_t n_wanted) {
    if (threadIdx.x == 0) top_begin(head->sel, n_wanted, head->counts[TOP_C_NUMBERS]);
}

// slab[blockIdx.x][256]: by digit d, the candidates whose higher digits equal the prefix.  A wave takes SWEEP_LINES x 64 consecutive
// lines a trip, their flags and then their keys loaded together: one line per lane and trip left the sweep waiting for one load after
// the other, 34 us where the bytes take 8 (profiles/top_lines.txt).  A wave whose counted lanes all hold the same digit -- small
// numbers share every high digit -- adds once; else every lane adds for itself.
__global__ void __launch_bounds__(256) k_top_hist(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cand, uint64_t n,
                                                  const TopDev* __restrict__ head, uint32_t d, uint32_t* __restrict__ slab) {
    __shared__ uint32_t h[TOP_BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t prefix = head->sel.prefix;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u * SWEEP_LINES;
    if (head->sel.n_top != 0u) {
        for (uint64_t i0 = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)) * SWEEP_LINES; i0 < n; i0 += stride) {
            uint8_t c[SWEEP_LINES];
            uint64_t key[SWEEP_LINES];
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_LINES; ++u) {
                const uint64_t i = i0 + u * 64u + lane;
                c[u] = i < n ? cand[i] : 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_LINES; ++u) key[u] = c[u] ? keys[i0 + u * 64u + lane] : 0ull;
#pragma unroll
            for (uint32_t u = 0; u < SWEEP_LINES; ++u) {
                const bool counted = c[u] != 0 && top_in_prefix(key[u], prefix, d);
                const uint32_t dg = top_digit(key[u], d);
                const uint64_t m = __ballot(counted);
                if (m != 0ull) {   // (the same in every lane of the wave)
                    const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(m))) - 1u;
                    const uint32_t wd = static_cast<uint32_t>(__shfl(static_cast<int>(dg), static_cast<int>(l)));
                    if (__ballot(counted && dg == wd) == m) {
                        if (lane == l) atomicAdd(&h[wd], static_cast<uint32_t>(__popcll(m)));
                    } else if (counted) {
                        atomicAdd(&h[dg], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    slab[static_cast<uint64_t>(blockIdx.x) * TOP_BINS + threadIdx.x] = h[threadIdx.x];
}

// one wave: digit d's step on the select's state
__global__ void __launch_bounds__(64) k_top_pick(TopDev* __restrict__ head, uint32_t d) {
    __shared__ uint32_t h[TOP_BINS];
    for (uint32_t q = threadIdx.x; q < TOP_BINS; q += 64u) h[q] = head->hist[q];
    __syncthreads();
    if (threadIdx.x == 0) top_step(head->sel, h, d);
}

// col[i] = 1 for a candidate above T, 2^32 for one equal to T, else 0: one scan of the column counts both kinds before every line
__global__ void __launch_bounds__(256) k_top_flags(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cand, uint64_t n,
                                                   const TopDev* __restrict__ head, uint64_t* __restrict__ col) {
    const uint64_t T = head->sel.prefix;
    const bool any = head->sel.n_top != 0u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        uint64_t f = 0;
        if (any && cand[i]) {
            const uint64_t key = keys[i];
            f = key > T ? 1ull : key == T ? (1ull << 32) : 0ull;
        }
        col[i] = f;
    }
}

// The chosen candidates as (key, line) pairs in line order: the chosen ones before line i are the keys above T before it and the
// first `remaining` of the keys equal to T.
__global__ void __launch_bounds__(256) k_top_compact(const uint64_t* __restrict__ col, const uint64_t* __restrict__ before, const uint64_t* __restrict__ keys,
                                                     uint64_t n, const TopDev* __restrict__ head, uint64_t* __restrict__ ckeys, uint32_t* __restrict__ clines) {
    const TopSelect s = head->sel;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint64_t f = col[i];
        if (f == 0ull) continue;
        const uint64_t b = before[i], above = b & 0xFFFFFFFFull, equal = b >> 32;
        const uint64_t key = keys[i];
        if (!top_chosen(s, key, equal)) continue;
        const uint64_t at = above + (equal < s.remaining ? equal : s.remaining);
        if (at < s.n_top && at < TOP_MAX_LINES) {   // (it is, by the select: n_top pairs in all)
            ckeys[at] = key;
            clines[at] = static_cast<uint32_t>(i);
        }
    }
}

// The n_top pairs by (key descending, place in the list ascending), by counting: rank = keys above + equal keys at a lower index,
// visibly stable.  Every workgroup keeps ALL the keys in LDS (32 KiB) and ranks ORDER_THREADS of the pairs, one per lane, walking the
// keys once: the list is in line order, so before the lane's own place a key counts when it is >= the lane's, behind it when it is >.
// (One workgroup ranking all 4 096 pairs took 0.6 ms of the call, 16 waves queueing on one CU: profiles/top_lines.txt.)
// plen[n_top .. n_wanted) = 0 for the scan behind it.
template <typename OFF>
__global__ void __launch_bounds__(ORDER_THREADS) k_top_order(const uint64_t* __restrict__ ckeys, const uint32_t* __restrict__ clines, const TopDev* __restrict__ head,
                                                             const OFF* __restrict__ off, uint32_t smallest, uint32_t n_wanted, uint32_t* __restrict__ perm,
                                                             int64_t* __restrict__ values, uint32_t* __restrict__ plen) {
    __shared__ uint64_t s_key[TOP_MAX_LINES];
    const uint32_t m = head->sel.n_top < TOP_MAX_LINES ? head->sel.n_top : TOP_MAX_LINES;
    const uint32_t at = blockIdx.x * ORDER_THREADS + threadIdx.x;
    if (blockIdx.x * ORDER_THREADS < m) {   // (the same in every lane of the workgroup)
        for (uint32_t j = threadIdx.x; j < m; j += ORDER_THREADS) s_key[j] = ckeys[j];
        __syncthreads();
        if (at < m) {
            const uint64_t mine = s_key[at];
            uint32_t rank = 0;
#pragma unroll 8
            for (uint32_t j = 0; j < at; ++j) rank += s_key[j] >= mine ? 1u : 0u;
#pragma unroll 8
            for (uint32_t j = at + 1u; j < m; ++j) rank += s_key[j] > mine ? 1u : 0u;
            const uint32_t line = clines[at];   // (rank < m: the ranks are a permutation of 0 .. m - 1)
            perm[rank] = line;
            values[rank] = top_value(mine, smallest != 0u);
            plen[rank] = static_cast<uint32_t>(static_cast<uint64_t>(off[line + 1u]) - static_cast<uint64_t>(off[line]));
        }
    }
    if (at >= m && at < n_wanted) plen[at] = 0u;
}

template <typename OFF, typename UNIT, bool NUM>
void launch_keys_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                    const TopArgs& a, const TopWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *ti = static_cast<const uint4*>(a.image), *wi = static_cast<const uint4*>(a.where_image);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_top_keys<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, ti, wi,
                           a.where_image_bytes, w.keys, w.cand, w.slab);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_top_keys<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, ti, wi,
                           a.where_image_bytes, w.keys, w.cand, w.slab);
    else
        hipLaunchKernelGGL((k_top_keys<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, ti, wi,
                           a.where_image_bytes, w.keys, w.cand, w.slab);
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint32_t keys_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, 2048)); }
uint32_t sweep_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 256u * SWEEP_LINES - 1) / (256u * SWEEP_LINES), 1024)); }

}  // namespace

TopWs top_workspace(void* ws, uint64_t n) {
    TopWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.head = take(sizeof(TopDev));
    w.slab = reinterpret_cast<uint32_t*>(take(std::max<uint64_t>(static_cast<uint64_t>(keys_blocks(n)) * TOP_COUNTS, static_cast<uint64_t>(sweep_blocks(n)) * TOP_BINS) * 4));
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n), scan_sums_bytes(TOP_MAX_LINES))));
    w.keys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.col = reinterpret_cast<uint64_t*>(take(n * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.ckeys = reinterpret_cast<uint64_t*>(take(TOP_MAX_LINES * 8));
    w.values = reinterpret_cast<int64_t*>(take(TOP_MAX_LINES * 8));
    w.dst_off = reinterpret_cast<uint64_t*>(take((TOP_MAX_LINES + 1) * 8));
    w.clines = reinterpret_cast<uint32_t*>(take(TOP_MAX_LINES * 4));
    w.perm = reinterpret_cast<uint32_t*>(take(TOP_MAX_LINES * 4));
    w.plen = reinterpret_cast<uint32_t*>(take(TOP_MAX_LINES * 4));
    w.cand = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t top_workspace_bytes(uint64_t n) { return top_workspace(nullptr, n).bytes; }

uint32_t top_keys_blocks(uint64_t n) { return keys_blocks(n); }

// The keys pass and the sum of its class counts, on `stream`; n > 0, parts > 0.  Of the workspace it uses keys, cand and slab (room for
// top_keys_blocks(n) * TOP_COUNTS words); counts[TOP_COUNTS] is on the device.
hipError_t launch_top_keys(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                           const TopWs& w, uint32_t* counts, hipStream_t stream) {
    const uint32_t lds = static_cast<uint32_t>(sizeof(TopHead)) + a.where_image_bytes;
    if (lds > 60u * 1024u) return hipErrorInvalidValue;   // (64 terms of 255 two-byte units: 35 KiB)
    const unsigned kb = keys_blocks(n);
    // (a.formats: a value group or a term reads a group under another number format than LONG -- the instantiation with the wider parser)
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (a.formats) launch_keys_as<OFF, UNIT, true>(fmt, kb, lds, stream, ids, row_units, K, n, offsets, a, w);
        else launch_keys_as<OFF, UNIT, false>(fmt, kb, lds, stream, ids, row_units, K, n, offsets, a, w);
    };
    if (a.wide) {
        if (offsets64) go(uint64_t{}, uint16_t{});
        else go(uint32_t{}, uint16_t{});
    } else {
        if (offsets64) go(uint64_t{}, uint8_t{});
        else go(uint32_t{}, uint8_t{});
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_top_sum, dim3(TOP_COUNTS), dim3(256), 0, stream, w.slab, kb, TOP_COUNTS, counts);
    return hipGetLastError();
}

// Every pass before the emit, on `stream`; n > 0, parts > 0, n_wanted <= TOP_MAX_LINES.  Leaves the class counts and the select's
// state at the workspace's head, and for n_wanted > 0: w.before[n] (its upper half: the candidates equal to T), w.perm, w.values and
// w.dst_off[0 .. n_wanted] (entries from n_top on: the units of all delivered lines).
hipError_t launch_top_select(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                             const TopWs& w, hipStream_t stream) {
    TopDev* head = reinterpret_cast<TopDev*>(w.head);
    hipError_t e = hipMemsetAsync(head, 0, sizeof(TopDev), stream);
    if (e != hipSuccess) return e;
    if (a.n_wanted > TOP_MAX_LINES) return hipErrorInvalidValue;
    e = launch_top_keys(ids, fmt, row_units, K, n, offsets, offsets64, a, w, head->counts, stream);
    if (e != hipSuccess) return e;
    if (a.n_wanted == 0u) return hipSuccess;
    const unsigned kb = keys_blocks(n);
    hipLaunchKernelGGL(k_top_begin, dim3(1), dim3(64), 0, stream, head, a.n_wanted);
    const unsigned sb = sweep_blocks(n);
    for (uint32_t d = TOP_DIGITS; d-- > 0u;) {
        hipLaunchKernelGGL(k_top_hist, dim3(sb), dim3(256), 0, stream, w.keys, w.cand, n, head, d, w.slab);
        hipLaunchKernelGGL(k_top_sum, dim3(TOP_BINS), dim3(256), 0, stream, w.slab, sb, TOP_BINS, head->hist);
        hipLaunchKernelGGL(k_top_pick, dim3(1), dim3(64), 0, stream, head, d);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_top_flags, dim3(kb), dim3(256), 0, stream, w.keys, w.cand, n, head, w.col);
    e = launch_exclusive_scan<uint64_t>(w.col, n, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_top_compact, dim3(kb), dim3(256), 0, stream, w.col, w.before, w.keys, n, head, w.ckeys, w.clines);
    const unsigned ob = (a.n_wanted + ORDER_THREADS - 1u) / ORDER_THREADS;
    if (offsets64)
        hipLaunchKernelGGL(k_top_order<uint64_t>, dim3(ob), dim3(ORDER_THREADS), 0, stream, w.ckeys, w.clines, head, static_cast<const uint64_t*>(offsets),
                           a.smallest, a.n_wanted, w.perm, w.values, w.plen);
    else
        hipLaunchKernelGGL(k_top_order<uint32_t>, dim3(ob), dim3(ORDER_THREADS), 0, stream, w.ckeys, w.clines, head, static_cast<const uint32_t*>(offsets),
                           a.smallest, a.n_wanted, w.perm, w.values, w.plen);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.plen, a.n_wanted, w.block_sums, w.dst_off, stream);
}

}  // namespace gx
