// gx_top_groups.hip -- the passes of gx_top_groups / gx_text_top_groups: the keys of a finished batch ranked by their lines or by the
// numbers their lines captured, on the device.  The reference's caller does this on the map it fills behind the extraction
// (README.md:26,63-79): byPath.entrySet().stream().sorted(comparingByValue().reversed()).limit(10).
// The rule -- the rank value, the key, the digit plan, the select step -- is gx_top_groups.hpp; the keys are gx_group_lines'
// (launch_group_build: build, flags, scans; its emit of all keys is not run).  DESIGN.md section 5.4.
//
//   keys     one lane per key, reached through the flagged first lines or through the slots, whichever reads less: the key's (hi, lo), a
//            candidate flag, its first line and slot, all indexed by key number.  The candidates' count and the OR and AND of both key
//            words are reduced by a butterfly per wave, LDS per workgroup, a slab per workgroup and the one-workgroup k_tg_begin,
//            which also makes the digit plan.
//   select   sixteen digits, most significant first, all launched; a digit that is not in the plan returns at once (its histogram
//            kernel writes nothing, its pick takes the digit from the OR).  A planned digit: k_tg_hist counts, by the digit, the
//            candidates under the prefix (LDS histogram per workgroup, a slab), k_tg_pick sums the slab in a fixed order and its
//            first lane applies tg_step.  The host reads nothing in between.  A key column that one histogram workgroup covers is
//            selected on by ONE launch, k_tg_select_one: the same steps as sixteen trips of a loop in one workgroup.
//   choose   k_tg_flags marks key > T and key == T, ONE scan counts both before every key number -- the two counts share a 64-bit
//            word -- and k_tg_compact writes the chosen (key, key number) entries in key-number order: the ties taken are the keys
//            that appeared first whatever the waves' timing.
//   order    rank = keys above + equal keys at a lower index, the chosen keys passing through LDS 2 048 at a time.  Leaves per rank
//            the key number, first line, slot and the key's length; a scan of the lengths gives the output offsets.
//   emit     one lane per rank writes the key's row and the slot's rank; its wave copies the key's units from the first line.
//            k_tg_line_rank maps slot_of through the per-slot ranks.
//
// No atomics in global memory anywhere, so every output has the same bits on every run.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group_dev.hpp"
#include "gx_scan.hpp"
#include "gx_top_groups.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t tg_smem[];

typedef unsigned long long u64;

constexpr uint32_t TG_ORDER_THREADS = 256;
constexpr uint32_t TG_ORDER_CHUNK = 2048;   // chosen keys in LDS at a time: 32 KiB
constexpr uint32_t TG_SWEEP_KEYS = 4;       // keys a lane of the histogram takes per trip
constexpr uint32_t TG_SLAB_WORDS = 5;       // a workgroup's candidates, OR hi, OR lo, AND hi, AND lo

__device__ __forceinline__ uint64_t tg_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }

// One lane per key.  by_slots == 0: lane i looks at line i < count = n and has a key when flags[i]; by_slots != 0: lane s looks at
// slot s < count = n_slots and has a key when the slot has lines.  The key's number is idx_off[its first line] < n_keys.
__global__ void __launch_bounds__(256) k_tg_keys(uint32_t by_slots, uint64_t count, uint64_t n, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ slot_of,
                                                 const uint64_t* __restrict__ idx_off, const u64* __restrict__ gw, const u64* __restrict__ gs, uint32_t rank_by,
                                                 uint32_t has_values, uint32_t smallest, uint64_t n_keys, uint64_t* __restrict__ key_hi, uint64_t* __restrict__ key_lo,
                                                 uint8_t* __restrict__ cand, uint32_t* __restrict__ first_of, uint32_t* __restrict__ slot_of_key,
                                                 uint64_t* __restrict__ slab) {
    __shared__ uint64_t s_part[4][TG_SLAB_WORDS];
    uint64_t cnt = 0, or_hi = 0, or_lo = 0, and_hi = ~0ull, and_lo = ~0ull;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < count; i += stride) {
        uint32_t slot = GROUP_NONE, first = 0;
        if (by_slots) {
            if (gw[i * GROUP_HEAD_WORDS + GROUP_W_LINES] != 0ull) {
                slot = static_cast<uint32_t>(i);
                first = group_first_line(gw[i * GROUP_HEAD_WORDS + GROUP_W_FIRST]);
            }
        } else if (flags[i] != 0) {
            slot = slot_of[i];
            first = static_cast<uint32_t>(i);
        }
        if (slot == GROUP_NONE || first >= n) continue;   // (a key's first line is a line of the batch)
        const uint64_t j = idx_off[first];
        if (j >= n_keys) continue;                        // (cannot be: the scan counted this very flag)
        int64_t hi = 0;
        uint64_t lo = 0;
        const bool c = tg_rank_value(rank_by, has_values != 0u, gw + static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS,
                                     gs + static_cast<uint64_t>(slot) * GROUP_STATS_WORDS, &hi, &lo);
        const TgKey k = tg_key(hi, lo, smallest != 0u);
        key_hi[j] = k.hi;
        key_lo[j] = k.lo;
        cand[j] = c ? 1 : 0;
        first_of[j] = first;
        slot_of_key[j] = slot;
        if (c) {
            ++cnt;
            or_hi |= k.hi; or_lo |= k.lo;
            and_hi &= k.hi; and_lo &= k.lo;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += tg_xor64(cnt, d);
        or_hi |= tg_xor64(or_hi, d); or_lo |= tg_xor64(or_lo, d);
        and_hi &= tg_xor64(and_hi, d); and_lo &= tg_xor64(and_lo, d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* p = s_part[threadIdx.x >> 6];
        p[0] = cnt; p[1] = or_hi; p[2] = or_lo; p[3] = and_hi; p[4] = and_lo;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t* out = slab + static_cast<uint64_t>(blockIdx.x) * TG_SLAB_WORDS;
        out[0] = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0];
        out[1] = s_part[0][1] | s_part[1][1] | s_part[2][1] | s_part[3][1];
        out[2] = s_part[0][2] | s_part[1][2] | s_part[2][2] | s_part[3][2];
        out[3] = s_part[0][3] & s_part[1][3] & s_part[2][3] & s_part[3][3];
        out[4] = s_part[0][4] & s_part[1][4] & s_part[2][4] & s_part[3][4];
    }
}

// one workgroup: the slabs joined, the select's first state and the digit plan
__global__ void __launch_bounds__(256) k_tg_begin(const uint64_t* __restrict__ slab, uint32_t blocks, uint32_t n_wanted, TgDev* __restrict__ head) {
    __shared__ uint64_t s_part[4][TG_SLAB_WORDS];
    uint64_t cnt = 0, or_hi = 0, or_lo = 0, and_hi = ~0ull, and_lo = ~0ull;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) {
        const uint64_t* p = slab + static_cast<uint64_t>(b) * TG_SLAB_WORDS;
        cnt += p[0];
        or_hi |= p[1]; or_lo |= p[2];
        and_hi &= p[3]; and_lo &= p[4];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += tg_xor64(cnt, d);
        or_hi |= tg_xor64(or_hi, d); or_lo |= tg_xor64(or_lo, d);
        and_hi &= tg_xor64(and_hi, d); and_lo &= tg_xor64(and_lo, d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* p = s_part[threadIdx.x >> 6];
        p[0] = cnt; p[1] = or_hi; p[2] = or_lo; p[3] = and_hi; p[4] = and_lo;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        head->candidates = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0];
        head->key_or = TgKey{s_part[0][1] | s_part[1][1] | s_part[2][1] | s_part[3][1], s_part[0][2] | s_part[1][2] | s_part[2][2] | s_part[3][2]};
        head->key_and = TgKey{s_part[0][3] & s_part[1][3] & s_part[2][3] & s_part[3][3], s_part[0][4] & s_part[1][4] & s_part[2][4] & s_part[3][4]};
        head->spare = 0;
        tg_begin(head->sel, n_wanted, head->candidates, head->key_or, head->key_and);
    }
}

// slab[blockIdx.x][256]: by digit d, the candidates whose higher digits equal the prefix.  A digit outside the plan: nothing.  A wave
// takes TG_SWEEP_KEYS x 64 consecutive keys a trip, their flags and then their words loaded together (k_top_hist's shape); a wave
// whose counted lanes all hold the same digit adds once.
__global__ void __launch_bounds__(256) k_tg_hist(const uint64_t* __restrict__ key_hi, const uint64_t* __restrict__ key_lo, const uint8_t* __restrict__ cand,
                                                 uint64_t n_keys, const TgDev* __restrict__ head, uint32_t d, uint32_t* __restrict__ slab) {
    __shared__ uint32_t h[TOP_BINS];
    const TgSelect sel = head->sel;
    if (!tg_planned(sel, d)) return;   // (the same in every lane of the grid)
    h[threadIdx.x] = 0u;
    __syncthreads();
    const TgKey prefix = sel.prefix;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u * TG_SWEEP_KEYS;
    for (uint64_t i0 = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)) * TG_SWEEP_KEYS; i0 < n_keys; i0 += stride) {
        uint8_t c[TG_SWEEP_KEYS];
        TgKey key[TG_SWEEP_KEYS];
#pragma unroll
        for (uint32_t u = 0; u < TG_SWEEP_KEYS; ++u) {
            const uint64_t i = i0 + u * 64u + lane;
            c[u] = i < n_keys ? cand[i] : 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < TG_SWEEP_KEYS; ++u) {
            const uint64_t i = i0 + u * 64u + lane;
            key[u] = c[u] ? TgKey{key_hi[i], key_lo[i]} : TgKey{0ull, 0ull};
        }
#pragma unroll
        for (uint32_t u = 0; u < TG_SWEEP_KEYS; ++u) {
            const bool counted = c[u] != 0 && tg_in_prefix(key[u], prefix, d);
            const uint32_t dg = tg_digit(key[u], d);
            const uint64_t m = __ballot(counted);
            if (m != 0ull) {   // (the same in every lane of the wave)
                const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(m))) - 1u;
                const uint32_t wd = static_cast<uint32_t>(__shfl(static_cast<int>(dg), static_cast<int>(l)));
                if (__ballot(counted && dg == wd) == m) {
                    if (lane == l) atomicAdd(&h[wd], static_cast<uint32_t>(__popcll(m)));
                } else if (counted) {
                    atomicAdd(&h[dg], 1u);
                }
            }
        }
    }
    __syncthreads();
    slab[static_cast<uint64_t>(blockIdx.x) * TOP_BINS + threadIdx.x] = h[threadIdx.x];
}

// one workgroup: lane b sums bin b over the workgroups' slabs in a fixed order, then the first lane applies digit d's step
__global__ void __launch_bounds__(256) k_tg_pick(const uint32_t* __restrict__ slab, uint32_t blocks, TgDev* __restrict__ head, uint32_t d) {
    __shared__ uint32_t h[TOP_BINS];
    const bool planned = tg_planned(head->sel, d);   // (n_top and plan: no step changes them)
    if (planned) {
        uint32_t t = 0;   // (unsigned adds: any grouping gives the same sum; eight loads are in flight at a time)
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) t += slab[static_cast<uint64_t>(b) * TOP_BINS + threadIdx.x];
        h[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0u) tg_step(head->sel, h, d, head->key_or);
}

// The whole select in ONE workgroup, for key columns that a single histogram workgroup covers (n_keys <= 256 x TG_SWEEP_KEYS: "by
// verb", "by status"): the sixteen digits' k_tg_hist / k_tg_pick pairs are thirty-two launches that each wait for the one before, and
// here they are sixteen trips of a loop.  The same steps on the same state: per planned digit an LDS histogram of the candidates under
// the prefix, then the first lane's tg_step; a skipped digit costs the first lane's step alone.
__global__ void __launch_bounds__(256) k_tg_select_one(const uint64_t* __restrict__ key_hi, const uint64_t* __restrict__ key_lo, const uint8_t* __restrict__ cand,
                                                       uint64_t n_keys, TgDev* __restrict__ head) {
    __shared__ uint32_t h[TOP_BINS];
    __shared__ TgSelect s_sel;
    if (threadIdx.x == 0u) s_sel = head->sel;
    __syncthreads();
    const TgKey key_or = head->key_or;
    for (uint32_t d = TG_DIGITS; d-- > 0u;) {
        const bool planned = tg_planned(s_sel, d);   // (the same in every lane: read behind a barrier, changed behind the next)
        if (planned) {
            h[threadIdx.x] = 0u;
            __syncthreads();
            const TgKey prefix = s_sel.prefix;
            for (uint64_t j = threadIdx.x; j < n_keys; j += 256u) {
                if (!cand[j]) continue;
                const TgKey key{key_hi[j], key_lo[j]};
                if (tg_in_prefix(key, prefix, d)) atomicAdd(&h[tg_digit(key, d)], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0u) tg_step(s_sel, h, d, key_or);
        __syncthreads();
    }
    if (threadIdx.x == 0u) head->sel = s_sel;
}

// col[j] = 1 for a candidate above T, 2^32 for one equal to T, else 0: one scan of the column counts both kinds before every key
__global__ void __launch_bounds__(256) k_tg_flags(const uint64_t* __restrict__ key_hi, const uint64_t* __restrict__ key_lo, const uint8_t* __restrict__ cand,
                                                  uint64_t n_keys, const TgDev* __restrict__ head, uint64_t* __restrict__ col) {
    const TgKey T = head->sel.prefix;
    const bool any = head->sel.n_top != 0u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < n_keys; j += stride) {
        uint64_t f = 0;
        if (any && cand[j]) {
            const TgKey key{key_hi[j], key_lo[j]};
            f = tg_above(key, T) ? 1ull : tg_equal(key, T) ? (1ull << 32) : 0ull;
        }
        col[j] = f;
    }
}

// The chosen candidates as (key, key number) entries in key-number order: the chosen ones before key j are the keys above T before
// it and the first `remaining` of the keys equal to T.
__global__ void __launch_bounds__(256) k_tg_compact(const uint64_t* __restrict__ col, const uint64_t* __restrict__ before, const uint64_t* __restrict__ key_hi,
                                                    const uint64_t* __restrict__ key_lo, uint64_t n_keys, const TgDev* __restrict__ head, uint64_t* __restrict__ c_hi,
                                                    uint64_t* __restrict__ c_lo, uint32_t* __restrict__ c_num) {
    const TgSelect s = head->sel;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < n_keys; j += stride) {
        if (col[j] == 0ull) continue;
        const uint64_t b = before[j], above = b & 0xFFFFFFFFull, equal = b >> 32;
        const TgKey key{key_hi[j], key_lo[j]};
        if (!tg_chosen(s, key, equal)) continue;
        const uint64_t at = above + (equal < s.remaining ? equal : s.remaining);
        if (at < s.n_top && at < TG_MAX) {   // (it is, by the select: n_top entries in all)
            c_hi[at] = key.hi;
            c_lo[at] = key.lo;
            c_num[at] = static_cast<uint32_t>(j);
        }
    }
}

// The n_top entries by (key descending, place in the list ascending), by counting: rank = keys above + equal keys at a lower index,
// visibly stable.  The list is in key-number order, so before the lane's own place a key counts when it is >= the lane's, behind it
// when it is >.  Every workgroup ranks TG_ORDER_THREADS entries, one per lane, and walks all keys once, TG_ORDER_CHUNK at a time in
// LDS.  plen[n_top .. n_wanted) = 0 for the scan behind it.
__global__ void __launch_bounds__(TG_ORDER_THREADS) k_tg_order(const uint64_t* __restrict__ c_hi, const uint64_t* __restrict__ c_lo, const uint32_t* __restrict__ c_num,
                                                               const TgDev* __restrict__ head, const uint32_t* __restrict__ first_of,
                                                               const uint32_t* __restrict__ slot_of_key, const uint32_t* __restrict__ klen, uint32_t n_wanted,
                                                               uint32_t* __restrict__ r_num, uint32_t* __restrict__ r_first, uint32_t* __restrict__ r_slot,
                                                               uint32_t* __restrict__ plen) {
    __shared__ uint64_t s_hi[TG_ORDER_CHUNK], s_lo[TG_ORDER_CHUNK];
    const uint32_t m = head->sel.n_top < TG_MAX ? head->sel.n_top : TG_MAX;
    const uint32_t at = blockIdx.x * TG_ORDER_THREADS + threadIdx.x;
    if (blockIdx.x * TG_ORDER_THREADS < m) {   // (the same in every lane of the workgroup)
        const bool have = at < m;
        const TgKey mine = have ? TgKey{c_hi[at], c_lo[at]} : TgKey{0ull, 0ull};
        uint32_t rank = 0;
        for (uint32_t base = 0; base < m; base += TG_ORDER_CHUNK) {
            const uint32_t len = m - base < TG_ORDER_CHUNK ? m - base : TG_ORDER_CHUNK;
            __syncthreads();
            for (uint32_t q = threadIdx.x; q < len; q += TG_ORDER_THREADS) { s_hi[q] = c_hi[base + q]; s_lo[q] = c_lo[base + q]; }
            __syncthreads();
            if (have) {
#pragma unroll 4
                for (uint32_t q = 0; q < len; ++q) {
                    const TgKey k{s_hi[q], s_lo[q]};
                    const uint32_t j = base + q;
                    rank += (tg_above(k, mine) || (j < at && tg_equal(k, mine))) ? 1u : 0u;
                }
            }
        }
        if (have && rank < m) {   // (the ranks are a permutation of 0 .. m - 1)
            const uint32_t j = c_num[at], first = first_of[j];
            r_num[rank] = j;
            r_first[rank] = first;
            r_slot[rank] = slot_of_key[j];
            plen[rank] = klen[first];
        }
    }
    if (at >= m && at < n_wanted) plen[at] = 0u;
}

// One lane per rank writes the key's row; its wave copies the key's units.  n_top / units_top: the totals the host has checked against
// the capacities, so nothing is written outside [0, n_top) and [0, units_top).
template <typename OFF, RowFormat F, typename UNIT>
__global__ void __launch_bounds__(256) k_tg_emit(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                 uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                 const uint32_t* __restrict__ r_num, const uint32_t* __restrict__ r_first, const uint32_t* __restrict__ r_slot,
                                                 const uint32_t* __restrict__ plen, const uint64_t* __restrict__ dst_off, const u64* __restrict__ gw,
                                                 const u64* __restrict__ gs, uint32_t has_values, uint32_t* __restrict__ rank_of_slot, TopGroupsOut out, uint32_t n_top,
                                                 uint64_t units_top) {
    uint4* g_l = reinterpret_cast<uint4*>(tg_smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(tg_smem);
    const GroupBatch<OFF, F, UNIT> batch{ids, caps, row_units, slots, K, off, data, gh};
    const uint32_t lane = threadIdx.x & 63u;
    UNIT* dst_units = static_cast<UNIT*>(out.key_units);
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.key_offsets) {
        if (out.offsets64) static_cast<uint64_t*>(out.key_offsets)[n_top] = units_top;
        else static_cast<uint32_t*>(out.key_offsets)[n_top] = static_cast<uint32_t>(units_top);
    }
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    uint64_t src = 0, dst = 0;
    uint32_t units = 0;
    if (r < n_top) {
        const uint32_t j = r_num[r], first = r_first[r], slot = r_slot[r];
        dst = dst_off[r];
        if (rank_of_slot) rank_of_slot[slot] = r;
        if (out.key_number) out.key_number[r] = j;
        if (out.key_first_line) out.key_first_line[r] = first;
        if (out.key_lines) out.key_lines[r] = gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_LINES];
        if (out.key_offsets) {
            if (out.offsets64) static_cast<uint64_t*>(out.key_offsets)[r] = dst;
            else static_cast<uint32_t*>(out.key_offsets)[r] = static_cast<uint32_t>(dst);
        }
        if (out.key_stats && has_values) {
            uint64_t w[GROUP_STATS_WORDS], s[8];
#pragma unroll
            for (uint32_t q = 0; q < GROUP_STATS_WORDS; ++q) w[q] = gs[static_cast<uint64_t>(slot) * GROUP_STATS_WORDS + q];
            group_stats_out(w, s);
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) out.key_stats[static_cast<uint64_t>(r) * 8u + q] = s[q];
        }
        if (dst_units && first < n) {
            const UNIT* p = batch.key_of(first, units);
            units = plen[r];                                  // (the same number; the build pass kept it)
            if (dst + units > units_top) units = 0;           // (cannot be: the scan summed these very lengths)
            src = static_cast<uint64_t>(p - data);
        }
    }
    // the wave copies its keys one after the other, 64 units a step: reads [src, src + units), writes [dst, dst + units)
    uint64_t todo = __ballot(units != 0u);
    while (todo) {
        const int l = __ffsll(static_cast<u64>(todo)) - 1;
        const uint64_t s = static_cast<uint64_t>(__shfl(static_cast<u64>(src), l)), d = static_cast<uint64_t>(__shfl(static_cast<u64>(dst), l));
        const uint32_t u = static_cast<uint32_t>(__shfl(static_cast<int>(units), l));
        for (uint32_t q = lane; q < u; q += 64u) dst_units[d + q] = data[s + q];
        todo &= todo - 1ull;
    }
}

// line -> slot -> the rank of the slot's key (GROUP_NONE: not delivered): k_group_line_key's shape, on the per-slot column that
// gx_group_lines' emit would fill with key numbers and that this call's emit fills with ranks
__global__ void __launch_bounds__(256) k_tg_line_rank(uint64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ rank_of_slot,
                                                      uint32_t* __restrict__ line_rank) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_of[i];
        line_rank[i] = slot == GROUP_NONE ? GROUP_NONE : rank_of_slot[slot];
    }
}

template <typename OFF, typename UNIT>
void launch_emit_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                    const GroupArgs& a, const GroupWs& g, const TopGroupsWs& w, uint32_t* rank_of_slot, const TopGroupsOut& out, uint32_t n_top, uint64_t units_top) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4* gi = static_cast<const uint4*>(a.image);
    const u64 *gw = reinterpret_cast<const u64*>(g.head_words), *gs = reinterpret_cast<const u64*>(g.stats_words);
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead));
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_tg_emit<OFF, ROWS_U8, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.r_num, w.r_first,
                           w.r_slot, w.plen, w.dst_off, gw, gs, a.has_values, rank_of_slot, out, n_top, units_top);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_tg_emit<OFF, ROWS_U16, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.r_num, w.r_first,
                           w.r_slot, w.plen, w.dst_off, gw, gs, a.has_values, rank_of_slot, out, n_top, units_top);
    else
        hipLaunchKernelGGL((k_tg_emit<OFF, ROWS_DENSE, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.r_num, w.r_first,
                           w.r_slot, w.plen, w.dst_off, gw, gs, a.has_values, rank_of_slot, out, n_top, units_top);
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint32_t key_blocks(uint64_t count) { return static_cast<uint32_t>(std::min<uint64_t>((count + 255) / 256, 2048)); }
uint32_t hist_blocks(uint64_t n_keys) {
    // (at most 64: the one-workgroup pick walks the slab, and a million keys are 17 MB -- 64 workgroups read them in microseconds)
    return static_cast<uint32_t>(std::min<uint64_t>((n_keys + 256u * TG_SWEEP_KEYS - 1) / (256u * TG_SWEEP_KEYS), 64));
}

}  // namespace

// does the keys pass go through the slots?  It reads a byte per line, or a slot's two head words.
bool top_groups_by_slots(uint64_t n, uint32_t n_slots) { return static_cast<uint64_t>(n_slots) * GROUP_HEAD_WORDS * 8u < n; }

TopGroupsWs top_groups_workspace(void* ws, uint64_t n, uint32_t n_slots, uint64_t n_keys) {
    TopGroupsWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    const uint64_t kb = key_blocks(std::max<uint64_t>(n, n_slots));
    w.head = take(sizeof(TgDev));
    w.slab = take(std::max<uint64_t>(kb * TG_SLAB_WORDS * 8u, static_cast<uint64_t>(hist_blocks(n_keys)) * TOP_BINS * 4u));
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n_keys), scan_sums_bytes(TG_MAX))));
    w.key_hi = reinterpret_cast<uint64_t*>(take(n_keys * 8));
    w.key_lo = reinterpret_cast<uint64_t*>(take(n_keys * 8));
    w.col = reinterpret_cast<uint64_t*>(take(n_keys * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n_keys + 1) * 8));
    w.c_hi = reinterpret_cast<uint64_t*>(take(TG_MAX * 8));
    w.c_lo = reinterpret_cast<uint64_t*>(take(TG_MAX * 8));
    w.dst_off = reinterpret_cast<uint64_t*>(take((TG_MAX + 1) * 8));
    w.first_of = reinterpret_cast<uint32_t*>(take(n_keys * 4));
    w.slot_of_key = reinterpret_cast<uint32_t*>(take(n_keys * 4));
    w.c_num = reinterpret_cast<uint32_t*>(take(TG_MAX * 4));
    w.r_num = reinterpret_cast<uint32_t*>(take(TG_MAX * 4));
    w.r_first = reinterpret_cast<uint32_t*>(take(TG_MAX * 4));
    w.r_slot = reinterpret_cast<uint32_t*>(take(TG_MAX * 4));
    w.plen = reinterpret_cast<uint32_t*>(take(TG_MAX * 4));
    w.cand = take(n_keys);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t top_groups_workspace_bytes(uint64_t n, uint32_t n_slots, uint64_t n_keys) { return top_groups_workspace(nullptr, n, n_slots, n_keys).bytes; }

// Every pass before the emit, on `stream`, behind launch_group_build and the host's look at its totals: 0 < n_keys <= n as the host
// read it, the table not overflowed, n_wanted <= TG_MAX.  Leaves TgDev at w.head, and for n_wanted > 0: w.before[n_keys] (its upper
// half: the candidates equal to T), w.r_num / r_first / r_slot / plen and w.dst_off[0 .. n_wanted] (entries from n_top on: the units of
// all delivered keys).
hipError_t launch_top_groups_select(uint64_t n, const GroupArgs& a, const GroupWs& g, uint64_t n_keys, uint32_t rank_by, uint32_t smallest, uint32_t n_wanted,
                                    const TopGroupsWs& w, hipStream_t stream) {
    if (n_wanted > TG_MAX || rank_by >= TG_RANK_KINDS || n_keys == 0 || n_keys > n) return hipErrorInvalidValue;
    TgDev* head = reinterpret_cast<TgDev*>(w.head);
    const bool by_slots = top_groups_by_slots(n, g.n_slots);
    const uint64_t count = by_slots ? g.n_slots : n;
    const unsigned kb = key_blocks(count);
    uint64_t* slab64 = reinterpret_cast<uint64_t*>(w.slab);
    uint32_t* slab32 = reinterpret_cast<uint32_t*>(w.slab);
    hipLaunchKernelGGL(k_tg_keys, dim3(kb), dim3(256), 0, stream, by_slots ? 1u : 0u, count, n, g.flags, g.slot_of, g.idx_off, reinterpret_cast<const u64*>(g.head_words),
                       reinterpret_cast<const u64*>(g.stats_words), rank_by, a.has_values, smallest, n_keys, w.key_hi, w.key_lo, w.cand, w.first_of, w.slot_of_key,
                       slab64);
    hipLaunchKernelGGL(k_tg_begin, dim3(1), dim3(256), 0, stream, slab64, kb, n_wanted, head);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_wanted == 0u) return e;
    const unsigned hb = hist_blocks(n_keys), fb = key_blocks(n_keys);
    if (hb == 1u) {
        hipLaunchKernelGGL(k_tg_select_one, dim3(1), dim3(256), 0, stream, w.key_hi, w.key_lo, w.cand, n_keys, head);
    } else {
        for (uint32_t d = TG_DIGITS; d-- > 0u;) {
            hipLaunchKernelGGL(k_tg_hist, dim3(hb), dim3(256), 0, stream, w.key_hi, w.key_lo, w.cand, n_keys, head, d, slab32);
            hipLaunchKernelGGL(k_tg_pick, dim3(1), dim3(256), 0, stream, slab32, hb, head, d);
        }
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tg_flags, dim3(fb), dim3(256), 0, stream, w.key_hi, w.key_lo, w.cand, n_keys, head, w.col);
    e = launch_exclusive_scan<uint64_t>(w.col, n_keys, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tg_compact, dim3(fb), dim3(256), 0, stream, w.col, w.before, w.key_hi, w.key_lo, n_keys, head, w.c_hi, w.c_lo, w.c_num);
    const unsigned ob = (n_wanted + TG_ORDER_THREADS - 1u) / TG_ORDER_THREADS;
    hipLaunchKernelGGL(k_tg_order, dim3(ob), dim3(TG_ORDER_THREADS), 0, stream, w.c_hi, w.c_lo, w.c_num, head, w.first_of, w.slot_of_key, g.klen, n_wanted, w.r_num,
                       w.r_first, w.r_slot, w.plen);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.plen, n_wanted, w.block_sums, w.dst_off, stream);
}

// The emit on `stream`, behind launch_top_groups_select and the host's check of the capacities: n_top <= the per-key arrays' capacity,
// units_top <= key_units' capacity.  out.line_rank: n entries.
hipError_t launch_top_groups_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                  const GroupWs& g, const TopGroupsWs& w, const TopGroupsOut& out, uint32_t n_top, uint64_t units_top,
                                  hipStream_t stream) {
    if (n_top > TG_MAX) return hipErrorInvalidValue;
    uint32_t* rank_of_slot = out.line_rank ? g.keynum : nullptr;   // (the per-slot column gx_group_lines' emit keeps its key numbers in)
    if (rank_of_slot) {
        const hipError_t e = hipMemsetAsync(rank_of_slot, 0xFF, static_cast<size_t>(g.n_slots) * 4, stream);
        if (e != hipSuccess) return e;
    }
    const unsigned blocks = std::max(1u, (n_top + 255u) / 256u);   // (n_top == 0: the offsets' one entry)
    if (a.wide) {
        if (offsets64) launch_emit_as<uint64_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w, rank_of_slot, out, n_top, units_top);
        else launch_emit_as<uint32_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w, rank_of_slot, out, n_top, units_top);
    } else {
        if (offsets64) launch_emit_as<uint64_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w, rank_of_slot, out, n_top, units_top);
        else launch_emit_as<uint32_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w, rank_of_slot, out, n_top, units_top);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out.line_rank) return e;
    hipLaunchKernelGGL(k_tg_line_rank, dim3(key_blocks(n)), dim3(256), 0, stream, n, g.slot_of, rank_of_slot, out.line_rank);
    return hipGetLastError();
}

}  // namespace gx
