// gx_group.hip -- the passes of gx_group_lines / gx_text_group_lines: the lines of a finished batch grouped by the text they captured,
// on the device.  The reference's caller does this right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) byVerb.merge(r.asMap().get("verb"), 1L, Long::sum);
// The rule -- hash, slot word, find-or-insert -- is gx_group.hpp's; "a line counts" is gx_capture_stats' (gx_where_dev.hpp).
//
// 1. k_group_build: one lane per line, grid-stride, k_capture_stats' grid.  outcome -> part -> terms -> key pair -> hash -> find-or-insert
//    (a 64-bit compare-and-swap on the table in global memory); the line's slot goes to slot_of[i], its key's length to klen[i].  What a
//    line ADDS to its slot -- one line, the minimum of the line number, and with a value group the counts, min, max, lo, hi of StatsAcc --
//    is merged on chip before it reaches global memory: per distinct slot among the wave's 64 lines by ballot (and a butterfly only where
//    a slot has several lines), then per workgroup in an LDS table of GROUP_LDS_ENTRIES entries keyed by slot number that holds up to
//    GROUP_LDS_KEYS slots and is flushed once, at the end of the workgroup's loop.  A slot that finds the LDS table full adds to global
//    memory directly.  All merges are unsigned adds and maxima of 64-bit integers (gx_group.hpp: the words' forms), so the sums do not
//    depend on timing.  Which line represents a slot does; nothing delivered depends on it.
// 2. k_group_flags: flag[i] = slot_of[i] valid and the slot's first line is i; klen[i] stays only there.  Two exclusive scans
//    (gx_scan.hpp) give each first line's key number and each key's offset.
// 3. k_group_emit: every first line writes its key's row (first line, lines, offset, stats), the slot's key number, and its wave copies
//    the key's units, 64 units a step.  k_group_line_key maps slot_of through the per-slot key numbers.
// DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_dev.hpp"
#include "gx_outcome.hpp"
#include "gx_scan.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t group_smem[];

typedef unsigned long long u64;

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// the table in global memory: the policy of group_find_or_insert on the device
struct GroupDevTable {
    u64* words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t claim(uint32_t slot, uint64_t word) { return atomicCAS(words + slot, 0ull, static_cast<u64>(word)); }
};

// (what one slot receives: GroupAdd and group_add of gx_group_dev.hpp)

// LDS: GroupHead, the term image (wimage_bytes, 0: no terms), then keys[GROUP_LDS_ENTRIES], 4 words (used, spare), 4 totals (64-bit),
// and GROUP_LDS_ENTRIES x (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) 64-bit words.
// totals[0..3]: lines that count, lines whose key pair names no value, status bits (1: a line of 4 G units, 2: the table is full).
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_group_build(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                     uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                     const uint4* __restrict__ wimage, uint32_t wimage_bytes, u64* __restrict__ table, uint32_t n_slots,
                                                     u64* __restrict__ gw, u64* __restrict__ gs, uint32_t* __restrict__ slot_of, uint32_t* __restrict__ klen,
                                                     u64* __restrict__ totals) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(group_smem);
    uint4* g_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    uint4* w_l = reinterpret_cast<uint4*>(smem + sizeof(GroupHead));
    for (uint32_t q = threadIdx.x; q < (wimage_bytes >> 4); q += 256u) w_l[q] = wimage[q];
    uint32_t* l_keys = reinterpret_cast<uint32_t*>(smem + sizeof(GroupHead) + wimage_bytes);
    uint32_t* l_used = l_keys + GROUP_LDS_ENTRIES;
    u64* l_totals = reinterpret_cast<u64*>(l_used + 4);
    u64* l_words = l_totals + 4;
    constexpr uint32_t EW = GROUP_HEAD_WORDS + GROUP_STATS_WORDS;
#ifndef GX_GROUP_NO_LDS
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) l_keys[q] = GROUP_NONE;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES * EW; q += 256u) l_words[q] = 0ull;
#endif
    if (threadIdx.x < 4u) { l_used[threadIdx.x] = 0u; l_totals[threadIdx.x] = 0ull; }
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(smem);
    const WhereHead* wh = reinterpret_cast<const WhereHead*>(smem + sizeof(GroupHead));
    const UNIT* lits = reinterpret_cast<const UNIT*>(smem + sizeof(GroupHead) + sizeof(WhereHead));
    const uint32_t n_ext = gh->n_parts;
    const bool weak = (gh->flags & GROUP_WEAK_HASH) != 0u, values = gh->has_values != 0u;
    const uint32_t ext_lo = n_ext ? gh->ext[0] : 1u, ext_hi = n_ext ? gh->ext[n_ext - 1u] : 0u;
    const bool terms = wimage_bytes != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const GroupBatch<OFF, F, UNIT> batch{ids, caps, row_units, slots, K, off, data, gh};
    GroupDevTable tab{table};
    uint64_t t_lines = 0, t_unset = 0;   // (the same in every lane of the wave)
    uint32_t t_status = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        uint32_t e = n_ext;   // the line's place in ext[]; n_ext: the line does not count
        uint64_t o0 = 0, line_units = 0;
        if (valid) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            o0 = static_cast<uint64_t>(off[i]);
            const uint64_t len = static_cast<uint64_t>(off[i + 1]) - o0;
            if (len > 0xFFFFFFFFull) t_status |= 1u;        // (a line of 4 G code units, or offsets that go backwards: refused by the host)
            line_units = len > 0xFFFFFFFFull ? 0u : len;    // (no value is looked at in a line that is refused anyway)
            if (oc >= ext_lo && oc <= ext_hi) {             // (oc <= ext_hi < K: a matched extraction)
                e = where_find(gh->ext, n_ext, oc);
                if (e < n_ext && terms && !where_line_holds<F, UNIT, NUM>(wh, lits, oc, ids, caps, i, row_units, slots, data + o0, line_units)) e = n_ext;
            }
        }
        uint32_t slot = GROUP_NONE, kn = 0;
        uint32_t cls = 3u;   // 0: a number, 1: unset, 2: no number, 3: the line has no value to measure
        int64_t v = 0;
        bool no_key = false;
        if (e < n_ext) {
            const GroupPart part = gh->part[e];
            int32_t pb, pe;
            pair_of<F>(ids, caps, i, row_units, slots, part.key_group, pb, pe);
            if (!where_pair_set(pb, pe, line_units)) {
                no_key = true;
            } else {
                const UNIT* kp = data + o0 + static_cast<uint32_t>(pb);
                kn = static_cast<uint32_t>(pe - pb);
                const uint32_t me = static_cast<uint32_t>(i);
                slot = group_find_or_insert(tab, n_slots, group_hash(kp, kn, weak), me, kp, kn, [&](uint32_t rep, const UNIT* a, uint32_t an) {
                    if (rep == me) return true;
                    uint32_t bn = 0;
                    const UNIT* b = batch.key_of(rep, bn);
                    return group_same_key(a, an, b, bn);
                });
                if (slot == GROUP_NONE) { t_status |= 2u; kn = 0; }
                else if (part.value_group != GROUP_NO_VALUE) {
                    pair_of<F>(ids, caps, i, row_units, slots, part.value_group, pb, pe);
                    if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                    else cls = number_parse_packed<NUM>(NUM ? gh->fmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                }
            }
        }
        if (valid) { slot_of[i] = slot; klen[i] = kn; }
        t_lines += static_cast<uint64_t>(__popcll(__ballot(e < n_ext)));
        t_unset += static_cast<uint64_t>(__popcll(__ballot(no_key)));
        // the distinct slots among the wave's 64 lines: every slot's lowest lane gathers what its lines add
        GroupAdd add{};
        bool leader = false;
        uint64_t todo = __ballot(slot != GROUP_NONE);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint32_t ws = static_cast<uint32_t>(__shfl(static_cast<int>(slot), static_cast<int>(l)));
            const bool mine = slot == ws;
            const uint64_t members = __ballot(mine);
            uint64_t numbers = 0, unset = 0, not_numbers = 0, lo = 0, hi = 0, mn = 0, mx = 0;
            if (values) {
                const bool num = mine && cls == 0u;
                numbers = __ballot(num);
                unset = __ballot(mine && cls == 1u);
                not_numbers = __ballot(mine && cls == 2u);
                lo = num ? (static_cast<uint64_t>(v) & 0xFFFFFFFFull) : 0ull;
                hi = num ? static_cast<uint64_t>(stats_high(v)) : 0ull;   // (two's complement: adds as unsigned)
                mn = num ? group_min_word(v) : 0ull;
                mx = num ? group_max_word(v) : 0ull;
                if (numbers && (members & (members - 1ull))) {            // (several lines on the slot: a butterfly; one line has its own)
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        lo += wave_xor64(lo, d);
                        hi += wave_xor64(hi, d);
                        mn = umax64(mn, wave_xor64(mn, d));
                        mx = umax64(mx, wave_xor64(mx, d));
                    }
                }
            }
            if (lane == l) {
                leader = true;
                add.lines = static_cast<uint64_t>(__popcll(members));
                add.first = group_first_word(static_cast<uint32_t>(i));   // (the lowest lane holds the lowest line)
                add.numbers = static_cast<uint64_t>(__popcll(numbers));
                add.unset = static_cast<uint64_t>(__popcll(unset));
                add.not_numbers = static_cast<uint64_t>(__popcll(not_numbers));
                add.lo = lo; add.hi = hi; add.mn = mn; add.mx = mx;
            }
            todo &= ~members;
        }
        if (leader) {
#ifndef GX_GROUP_NO_LDS
            const uint32_t ent = group_lds_entry(l_keys, l_used, slot);
            if (ent != GROUP_NONE) {
                u64* w = l_words + ent * EW;
                group_add(w, w + GROUP_HEAD_WORDS, values, add);
            } else
#endif
            {
                // (the experiment's other arm, build.py --variant -DGX_GROUP_NO_LDS: every wave adds to global memory; profiles/group_lines.txt)
                group_add(gw + static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS, gs + static_cast<uint64_t>(slot) * GROUP_STATS_WORDS, values, add);
            }
        }
    }
    if (lane == 0u) {
        if (t_lines) atomicAdd(l_totals + 0, static_cast<u64>(t_lines));
        if (t_unset) atomicAdd(l_totals + 1, static_cast<u64>(t_unset));
    }
    // (status: every lane has its own bits)
    const uint64_t any1 = __ballot((t_status & 1u) != 0u), any2 = __ballot((t_status & 2u) != 0u);
    if (lane == 0u && (any1 | any2)) atomicOr(l_totals + 2, static_cast<u64>((any1 ? 1u : 0u) | (any2 ? 2u : 0u)));
    __syncthreads();
    if (threadIdx.x < 3u && l_totals[threadIdx.x]) {
        if (threadIdx.x == 2u) atomicOr(totals + 2, l_totals[2]);
        else atomicAdd(totals + threadIdx.x, l_totals[threadIdx.x]);
    }
#ifndef GX_GROUP_NO_LDS
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) {
        const uint32_t s = l_keys[q];
        if (s == GROUP_NONE) continue;
        const u64* w = l_words + q * EW;
        if (w[GROUP_W_LINES] == 0ull) continue;   // (claimed by a lane whose words went elsewhere: nothing to flush)
        const u64* st = w + GROUP_HEAD_WORDS;
        const GroupAdd a{w[GROUP_W_LINES], w[GROUP_W_FIRST], st[GROUP_S_NUMBERS], st[GROUP_S_UNSET], st[GROUP_S_NOT_NUMBERS], st[GROUP_S_MIN], st[GROUP_S_MAX],
                         st[GROUP_S_LO], st[GROUP_S_HI]};
        group_add(gw + static_cast<uint64_t>(s) * GROUP_HEAD_WORDS, gs + static_cast<uint64_t>(s) * GROUP_STATS_WORDS, values, a);
    }
#endif
}

// flag[i] = line i is the first line of its key; klen[i] stays only there
__global__ void __launch_bounds__(256) k_group_flags(uint64_t n, const uint32_t* __restrict__ slot_of, const u64* __restrict__ gw, uint8_t* __restrict__ flags,
                                                     uint32_t* __restrict__ klen) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_of[i];
        const bool first = slot != GROUP_NONE && group_first_line(gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_FIRST]) == static_cast<uint32_t>(i);
        flags[i] = first ? 1 : 0;
        if (!first) klen[i] = 0u;
    }
}

// Every first line writes its key's row and the slot's key number; its wave copies the key's units.  n_keys / key_units: the totals the
// host has checked against the capacities, so nothing is written outside [0, n_keys) and [0, key_units).
template <typename OFF, RowFormat F, typename UNIT>
__global__ void __launch_bounds__(256) k_group_emit(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                    uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                    const uint8_t* __restrict__ flags, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ klen,
                                                    const uint64_t* __restrict__ idx_off, const uint64_t* __restrict__ dst_off, const u64* __restrict__ gw,
                                                    const u64* __restrict__ gs, uint32_t* __restrict__ keynum, GroupOut out, uint64_t n_keys, uint64_t key_units) {
    uint4* g_l = reinterpret_cast<uint4*>(group_smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(group_smem);
    const GroupBatch<OFF, F, UNIT> batch{ids, caps, row_units, slots, K, off, data, gh};
    const uint32_t lane = threadIdx.x & 63u;
    UNIT* dst_units = static_cast<UNIT*>(out.key_units);
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.key_offsets) {
        if (out.offsets64) static_cast<uint64_t*>(out.key_offsets)[n_keys] = key_units;
        else static_cast<uint32_t*>(out.key_offsets)[n_keys] = static_cast<uint32_t>(key_units);
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool first = i < n && flags[i] != 0;
        uint64_t src = 0, dst = 0;
        uint32_t units = 0;
        if (first) {
            const uint64_t j = idx_off[i];
            const uint32_t slot = slot_of[i];
            dst = dst_off[i];
            if (j < n_keys) {
                keynum[slot] = static_cast<uint32_t>(j);
                if (out.key_first_line) out.key_first_line[j] = static_cast<uint32_t>(i);
                if (out.key_lines) out.key_lines[j] = gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_LINES];
                if (out.key_offsets) {
                    if (out.offsets64) static_cast<uint64_t*>(out.key_offsets)[j] = dst;
                    else static_cast<uint32_t*>(out.key_offsets)[j] = static_cast<uint32_t>(dst);
                }
                if (out.key_stats) {
                    uint64_t w[GROUP_STATS_WORDS], s[8];
#pragma unroll
                    for (uint32_t q = 0; q < GROUP_STATS_WORDS; ++q) w[q] = gs[static_cast<uint64_t>(slot) * GROUP_STATS_WORDS + q];
                    group_stats_out(w, s);
#pragma unroll
                    for (uint32_t q = 0; q < 8u; ++q) out.key_stats[j * 8u + q] = s[q];
                }
                if (dst_units) {
                    const UNIT* p = batch.key_of(static_cast<uint32_t>(i), units);
                    units = klen[i];                                  // (the same number; the pass before kept it)
                    if (dst + units > key_units) units = 0;           // (cannot be: the scan summed these very lengths)
                    src = static_cast<uint64_t>(p - data);
                }
            }
        }
        // the wave copies its first lines' keys one after the other, 64 units a step: reads [src, src + units), writes [dst, dst + units)
        uint64_t todo = __ballot(units != 0u);
        while (todo) {
            const int l = __ffsll(static_cast<u64>(todo)) - 1;
            const uint64_t s = static_cast<uint64_t>(__shfl(static_cast<u64>(src), l)), d = static_cast<uint64_t>(__shfl(static_cast<u64>(dst), l));
            const uint32_t u = static_cast<uint32_t>(__shfl(static_cast<int>(units), l));
            for (uint32_t q = lane; q < u; q += 64u) dst_units[d + q] = data[s + q];
            todo &= todo - 1ull;
        }
    }
}

__global__ void __launch_bounds__(256) k_group_line_key(uint64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ keynum,
                                                        uint32_t* __restrict__ line_key) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_of[i];
        line_key[i] = slot == GROUP_NONE ? GROUP_NONE : keynum[slot];
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_build_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const GroupArgs& a, const GroupWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *wi = static_cast<const uint4*>(a.where_image);
    u64 *table = reinterpret_cast<u64*>(w.table), *gw = reinterpret_cast<u64*>(w.head_words), *gs = reinterpret_cast<u64*>(w.stats_words),
        *totals = reinterpret_cast<u64*>(w.totals);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_group_build<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, w.klen, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_group_build<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, w.klen, totals);
    else
        hipLaunchKernelGGL((k_group_build<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, w.klen, totals);
}

template <typename OFF, typename UNIT>
void launch_emit_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                    const GroupArgs& a, const GroupWs& w, const GroupOut& out, uint64_t n_keys, uint64_t key_units) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4* gi = static_cast<const uint4*>(a.image);
    const u64 *gw = reinterpret_cast<const u64*>(w.head_words), *gs = reinterpret_cast<const u64*>(w.stats_words);
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead));
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_group_emit<OFF, ROWS_U8, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.flags,
                           w.slot_of, w.klen, w.idx_off, w.dst_off, gw, gs, w.keynum, out, n_keys, key_units);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_group_emit<OFF, ROWS_U16, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.flags,
                           w.slot_of, w.klen, w.idx_off, w.dst_off, gw, gs, w.keynum, out, n_keys, key_units);
    else
        hipLaunchKernelGGL((k_group_emit<OFF, ROWS_DENSE, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, w.flags,
                           w.slot_of, w.klen, w.idx_off, w.dst_off, gw, gs, w.keynum, out, n_keys, key_units);
}

unsigned group_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048)); }

}  // namespace

// The slots' words -- zeroed before every call by ONE memset -- and the per-slot key numbers: [table n_slots][head 2 n_slots]
// [stats 8 n_slots, with values][totals 8], all 64-bit, then keynum[n_slots].
size_t group_table_zero_bytes(uint32_t n_slots, bool values) {
    return (static_cast<size_t>(n_slots) * (1u + GROUP_HEAD_WORDS + (values ? GROUP_STATS_WORDS : 0u)) + 8u) * 8u;
}
size_t group_table_bytes(uint32_t n_slots, bool values) { return group_table_zero_bytes(n_slots, values) + static_cast<size_t>(n_slots) * 4u; }

static size_t up16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

// The per-line arrays: idx_off and dst_off (n + 1, 64-bit), the two scans' block sums, slot_of and klen (32-bit), flags.
size_t group_lines_bytes(uint64_t n) {
    return 2 * up16((n + 1) * 8) + 2 * scan_sums_bytes(n) + 2 * up16(n * 4) + up16(n);
}

GroupWs group_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, bool values) {
    GroupWs w{};
    w.n_slots = n_slots;
    uint64_t* t = static_cast<uint64_t*>(table_mem);
    w.table = t;
    w.head_words = t + n_slots;
    w.stats_words = w.head_words + static_cast<size_t>(n_slots) * GROUP_HEAD_WORDS;   // (never touched without values)
    w.totals = w.stats_words + (values ? static_cast<size_t>(n_slots) * GROUP_STATS_WORDS : 0u);
    w.keynum = reinterpret_cast<uint32_t*>(w.totals + 8);
    uint8_t* p = static_cast<uint8_t*>(lines_mem);
    w.idx_off = reinterpret_cast<uint64_t*>(p); p += up16((n + 1) * 8);
    w.dst_off = reinterpret_cast<uint64_t*>(p); p += up16((n + 1) * 8);
    w.sums_a = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n);
    w.sums_b = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n);
    w.slot_of = reinterpret_cast<uint32_t*>(p); p += up16(n * 4);
    w.klen = reinterpret_cast<uint32_t*>(p); p += up16(n * 4);
    w.flags = p;
    return w;
}

// Passes 1 and 2 on `stream`, n > 0 and parts > 0: leaves w.totals (lines, unset, status), w.idx_off[n] = the keys and w.dst_off[n] =
// their units.  The part image (and the term image, if any) are on the device.
hipError_t launch_group_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                              const GroupWs& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.table, 0, group_table_zero_bytes(w.n_slots, a.has_values != 0), stream);
    if (e != hipSuccess) return e;
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead)) + a.where_image_bytes + GROUP_LDS_ENTRIES * 4u + 16u + 32u +
                         GROUP_LDS_ENTRIES * (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) * 8u;
    if (lds > 64u * 1024u) return hipErrorInvalidValue;   // (64 terms of 255 two-byte units: 34 KiB; GroupHead and the LDS table: 11.1 KiB)
    const unsigned blocks = group_blocks(n);
    // (a.formats: a value group or a term reads a group under another number format than LONG -- the instantiation with the wider parser)
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (a.formats) launch_build_as<OFF, UNIT, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, w);
        else launch_build_as<OFF, UNIT, false>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, w);
    };
    if (a.wide) {
        if (offsets64) go(uint64_t{}, uint16_t{});
        else go(uint32_t{}, uint16_t{});
    } else {
        if (offsets64) go(uint64_t{}, uint8_t{});
        else go(uint32_t{}, uint8_t{});
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_flags, dim3(blocks), dim3(256), 0, stream, n, w.slot_of, reinterpret_cast<const u64*>(w.head_words), w.flags, w.klen);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(w.flags, n, w.sums_a, w.idx_off, stream);
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.klen, n, w.sums_b, w.dst_off, stream);
}

// Pass 3 on `stream`, behind launch_group_build and the host's check of the capacities: n_keys <= the per-key arrays' capacity and
// key_units <= key_units' capacity.
hipError_t launch_group_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                             const GroupWs& w, const GroupOut& out, uint64_t n_keys, uint64_t key_units, hipStream_t stream) {
    const unsigned blocks = group_blocks(n);
    if (a.wide) {
        if (offsets64) launch_emit_as<uint64_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w, out, n_keys, key_units);
        else launch_emit_as<uint32_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w, out, n_keys, key_units);
    } else {
        if (offsets64) launch_emit_as<uint64_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w, out, n_keys, key_units);
        else launch_emit_as<uint32_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w, out, n_keys, key_units);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out.line_key) return e;
    hipLaunchKernelGGL(k_group_line_key, dim3(blocks), dim3(256), 0, stream, n, w.slot_of, w.keynum, out.line_key);
    return hipGetLastError();
}

}  // namespace gx
