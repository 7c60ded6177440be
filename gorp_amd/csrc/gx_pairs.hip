// gx_pairs.hip -- the passes of gx_group_pairs / gx_text_group_pairs: the lines of a finished batch grouped by TWO captured texts, on the
// device.  The reference's caller does this right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) byBoth.merge(List.of(r.asMap().get("verb"), r.asMap().get("path")), 1L, Long::sum);
// The rule -- pair hash, pair equality, find-or-insert on gx_group.hpp's slot words -- is gx_pairs.hpp's.  All passes run behind
// launch_group_build (gx_group.hip), which leaves slot_of[] complete and is not changed: a line's key IS its key slot.
//
// 1. k_pairs_build: one lane per line, grid-stride, the build's grid.  Lines without a key slot are skipped; the others count and are
//    keyed, so no term is evaluated again.  outcome -> part -> second pair -> pair_hash -> find-or-insert (a 64-bit compare-and-swap on
//    the pair table in global memory); the line's pair slot goes to pslot_of[i], its second's length to plen[i].  What a line ADDS to
//    its pair slot -- one line and the minimum of the line number -- is merged on chip before it reaches global memory, exactly as
//    k_group_build does: per distinct pair slot among the wave's 64 lines by ballot, then per workgroup in an LDS table
//    (group_lds_entry, keyed by pair slot) that is flushed once.  All merges are unsigned adds and maxima of 64-bit integers.
// 2. k_pairs_flags: pflag[i] = line i is the first line of its pair; plen[i] stays only there.  Two exclusive scans (gx_scan.hpp) give
//    each first line's pair number and each pair's unit offset.  The same pass counts the pairs per KEY slot: every first-of-pair line
//    adds 1 to kpairs[slot_of[i]], merged per wave (ballot by key slot) and per workgroup (the same LDS table, keyed by key slot) first,
//    so six keys with millions of seconds each do not put millions of adds on six words.
// 3. k_pairs_emit, behind launch_group_emit (keynum[]): every first-of-pair line writes its pair's row (key number, first line, lines,
//    offset) and the pair slot's number, and its wave copies the second's units, 64 units a step; every first-of-KEY line writes
//    key_pairs.  k_pairs_line_pair maps pslot_of through the per-pair-slot numbers.
// DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_dev.hpp"
#include "gx_outcome.hpp"
#include "gx_pairs.hpp"
#include "gx_scan.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t pairs_smem[];

typedef unsigned long long u64;

// the pair table in global memory: the policy of group_find_or_insert on the device
struct PairsDevTable {
    u64* words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t claim(uint32_t slot, uint64_t word) { return atomicCAS(words + slot, 0ull, static_cast<u64>(word)); }
};

// a finished batch and its finished key slots as the pair passes read them
template <typename OFF, RowFormat F, typename UNIT>
struct PairsBatch {
    const void* ids;
    const int32_t* caps;
    uint32_t row_units, slots, K;
    const OFF* off;
    const UNIT* data;
    const GroupHead* gh;       // in LDS
    const PairsHead* ph;       // in LDS
    const uint32_t* slot_of;   // launch_group_build's

    // The key slot and the second of line r, which IS paired (its part has a second group and that group's pair is set).
    __device__ __forceinline__ const UNIT* pair_of_line(uint32_t r, uint32_t& key_slot, uint32_t& units) const {
        const uint32_t oc = outcome_of(id_of<F>(ids, r, row_units), K);
        const uint32_t e = where_find(gh->ext, gh->n_parts, oc);
        const int32_t sg = ph->second[e < gh->n_parts ? e : 0u];
        int32_t pb, pe;
        pair_of<F>(ids, caps, r, row_units, slots, static_cast<uint32_t>(sg < 0 ? 0 : sg), pb, pe);
        units = static_cast<uint32_t>(pe - pb);
        key_slot = slot_of[r];
        return data + static_cast<uint64_t>(off[r]) + static_cast<uint32_t>(pb);
    }
};

__device__ __forceinline__ void pairs_add(u64* head, uint64_t lines, uint64_t first) {
    atomicAdd(head + GROUP_W_LINES, static_cast<u64>(lines));
    atomicMax(head + GROUP_W_FIRST, static_cast<u64>(first));
}

// LDS: GroupHead, PairsHead, then keys[GROUP_LDS_ENTRIES], 4 words (used, spare), 4 totals (64-bit), and GROUP_LDS_ENTRIES x
// GROUP_HEAD_WORDS 64-bit words.  totals[0..2]: paired lines, unpaired lines, status bits (2: the pair table is full).
template <typename OFF, RowFormat F, typename UNIT>
__global__ void __launch_bounds__(256) k_pairs_build(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                     uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                     const uint4* __restrict__ pimage, const uint32_t* __restrict__ slot_of, u64* __restrict__ table,
                                                     uint32_t n_slots, u64* __restrict__ pw, uint32_t* __restrict__ pslot_of, uint32_t* __restrict__ plen,
                                                     u64* __restrict__ totals) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(pairs_smem);
    uint4* g_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    uint4* p_l = reinterpret_cast<uint4*>(smem + sizeof(GroupHead));
    for (uint32_t q = threadIdx.x; q < (sizeof(PairsHead) >> 4); q += 256u) p_l[q] = pimage[q];
    uint32_t* l_keys = reinterpret_cast<uint32_t*>(smem + sizeof(GroupHead) + sizeof(PairsHead));
    uint32_t* l_used = l_keys + GROUP_LDS_ENTRIES;
    u64* l_totals = reinterpret_cast<u64*>(l_used + 4);
    u64* l_words = l_totals + 4;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) l_keys[q] = GROUP_NONE;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES * GROUP_HEAD_WORDS; q += 256u) l_words[q] = 0ull;
    if (threadIdx.x < 4u) { l_used[threadIdx.x] = 0u; l_totals[threadIdx.x] = 0ull; }
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(smem);
    const PairsHead* ph = reinterpret_cast<const PairsHead*>(smem + sizeof(GroupHead));
    const uint32_t n_ext = gh->n_parts;
    const bool weak = (gh->flags & GROUP_WEAK_HASH) != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const PairsBatch<OFF, F, UNIT> batch{ids, caps, row_units, slots, K, off, data, gh, ph, slot_of};
    PairsDevTable tab{table};
    uint64_t t_paired = 0, t_unpaired = 0;   // (the same in every lane of the wave)
    bool t_full = false;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        const uint32_t kslot = valid ? slot_of[i] : GROUP_NONE;
        const bool keyed = kslot != GROUP_NONE;   // (the line counts and its key pair is set: the build found it so)
        uint32_t pslot = GROUP_NONE, sn = 0;
        if (keyed) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            const uint32_t e = where_find(gh->ext, n_ext, oc);
            const int32_t sg = e < n_ext ? ph->second[e] : PAIRS_NO_SECOND;
            if (sg >= 0) {
                const uint64_t o0 = static_cast<uint64_t>(off[i]);
                const uint64_t line_units = static_cast<uint64_t>(off[i + 1]) - o0;   // (< 4 G: the build gives no key to a longer line)
                int32_t pb, pe;
                pair_of<F>(ids, caps, i, row_units, slots, static_cast<uint32_t>(sg), pb, pe);
                if (where_pair_set(pb, pe, line_units)) {
                    const UNIT* sp = data + o0 + static_cast<uint32_t>(pb);
                    sn = static_cast<uint32_t>(pe - pb);
                    pslot = pair_find_or_insert(tab, n_slots, kslot, static_cast<uint32_t>(i), sp, sn, weak,
                                                [&](uint32_t rep, uint32_t& rs, uint32_t& rn) { return batch.pair_of_line(rep, rs, rn); });
                    if (pslot == GROUP_NONE) { t_full = true; sn = 0; }
                }
            }
        }
        if (valid) { pslot_of[i] = pslot; plen[i] = sn; }
        t_paired += static_cast<uint64_t>(__popcll(__ballot(pslot != GROUP_NONE)));
        t_unpaired += static_cast<uint64_t>(__popcll(__ballot(keyed && pslot == GROUP_NONE)));
        // the distinct pair slots among the wave's 64 lines: every slot's lowest lane gathers what its lines add
        uint64_t add_lines = 0;
        bool leader = false;
        uint64_t todo = __ballot(pslot != GROUP_NONE);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint32_t ws = static_cast<uint32_t>(__shfl(static_cast<int>(pslot), static_cast<int>(l)));
            const uint64_t members = __ballot(pslot == ws);
            if (lane == l) {
                leader = true;
                add_lines = static_cast<uint64_t>(__popcll(members));
            }
            todo &= ~members;
        }
        if (leader) {
            const uint64_t first = group_first_word(static_cast<uint32_t>(i));   // (the lowest lane holds the lowest line)
            const uint32_t ent = group_lds_entry(l_keys, l_used, pslot);
            if (ent != GROUP_NONE) pairs_add(l_words + ent * GROUP_HEAD_WORDS, add_lines, first);
            else pairs_add(pw + static_cast<uint64_t>(pslot) * GROUP_HEAD_WORDS, add_lines, first);
        }
    }
    if (lane == 0u) {
        if (t_paired) atomicAdd(l_totals + 0, static_cast<u64>(t_paired));
        if (t_unpaired) atomicAdd(l_totals + 1, static_cast<u64>(t_unpaired));
    }
    const uint64_t any_full = __ballot(t_full);   // (every lane has its own)
    if (lane == 0u && any_full) atomicOr(l_totals + 2, static_cast<u64>(2u));
    __syncthreads();
    if (threadIdx.x < 3u && l_totals[threadIdx.x]) {
        if (threadIdx.x == 2u) atomicOr(totals + 2, l_totals[2]);
        else atomicAdd(totals + threadIdx.x, l_totals[threadIdx.x]);
    }
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) {
        const uint32_t s = l_keys[q];
        if (s == GROUP_NONE) continue;
        const u64* w = l_words + q * GROUP_HEAD_WORDS;
        if (w[GROUP_W_LINES] == 0ull) continue;   // (claimed by a lane whose words went elsewhere: nothing to flush)
        pairs_add(pw + static_cast<uint64_t>(s) * GROUP_HEAD_WORDS, w[GROUP_W_LINES], w[GROUP_W_FIRST]);
    }
}

// pflag[i] = line i is the first line of its pair; plen[i] stays only there; kpairs[key slot] += 1 per first-of-pair line, merged per
// wave and per workgroup first
__global__ void __launch_bounds__(256) k_pairs_flags(uint64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ pslot_of,
                                                     const u64* __restrict__ pw, uint8_t* __restrict__ flags, uint32_t* __restrict__ plen, u64* __restrict__ kpairs) {
    __shared__ uint32_t l_keys[GROUP_LDS_ENTRIES];
    __shared__ uint32_t l_used[4];
    __shared__ u64 l_count[GROUP_LDS_ENTRIES];
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) { l_keys[q] = GROUP_NONE; l_count[q] = 0ull; }
    if (threadIdx.x < 4u) l_used[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        const uint32_t pslot = valid ? pslot_of[i] : GROUP_NONE;
        const bool first = pslot != GROUP_NONE && group_first_line(pw[static_cast<uint64_t>(pslot) * GROUP_HEAD_WORDS + GROUP_W_FIRST]) == static_cast<uint32_t>(i);
        if (valid) {
            flags[i] = first ? 1 : 0;
            if (!first) plen[i] = 0u;
        }
        const uint32_t kslot = first ? slot_of[i] : GROUP_NONE;   // (a paired line has a key slot)
        uint64_t count = 0;
        bool leader = false;
        uint64_t todo = __ballot(kslot != GROUP_NONE);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint32_t ws = static_cast<uint32_t>(__shfl(static_cast<int>(kslot), static_cast<int>(l)));
            const uint64_t members = __ballot(kslot == ws);
            if (lane == l) {
                leader = true;
                count = static_cast<uint64_t>(__popcll(members));
            }
            todo &= ~members;
        }
        if (leader) {
            const uint32_t ent = group_lds_entry(l_keys, l_used, kslot);
            if (ent != GROUP_NONE) atomicAdd(l_count + ent, static_cast<u64>(count));
            else atomicAdd(kpairs + kslot, static_cast<u64>(count));
        }
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) {
        const uint32_t s = l_keys[q];
        if (s != GROUP_NONE && l_count[q] != 0ull) atomicAdd(kpairs + s, l_count[q]);
    }
}

// Every first-of-pair line writes its pair's row and the pair slot's number; its wave copies the second's units.  Every first-of-key
// line writes its key's pairs.  n_pairs / pair_units / n_keys: the totals the host has checked against the capacities, so nothing is
// written outside [0, n_pairs), [0, pair_units) and [0, n_keys).
template <typename OFF, RowFormat F, typename UNIT>
__global__ void __launch_bounds__(256) k_pairs_emit(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                    uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                    const uint4* __restrict__ pimage, const uint32_t* __restrict__ slot_of, const uint8_t* __restrict__ kflags,
                                                    const uint64_t* __restrict__ kidx_off, const uint32_t* __restrict__ keynum, const uint8_t* __restrict__ flags,
                                                    const uint32_t* __restrict__ pslot_of, const uint32_t* __restrict__ plen, const uint64_t* __restrict__ idx_off,
                                                    const uint64_t* __restrict__ dst_off, const u64* __restrict__ pw, const u64* __restrict__ kpairs,
                                                    uint32_t* __restrict__ pairnum, PairsOut out, uint64_t n_pairs, uint64_t pair_units, uint64_t n_keys) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(pairs_smem);
    uint4* g_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    uint4* p_l = reinterpret_cast<uint4*>(smem + sizeof(GroupHead));
    for (uint32_t q = threadIdx.x; q < (sizeof(PairsHead) >> 4); q += 256u) p_l[q] = pimage[q];
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(smem);
    const PairsHead* ph = reinterpret_cast<const PairsHead*>(smem + sizeof(GroupHead));
    const PairsBatch<OFF, F, UNIT> batch{ids, caps, row_units, slots, K, off, data, gh, ph, slot_of};
    const uint32_t lane = threadIdx.x & 63u;
    UNIT* dst_units = static_cast<UNIT*>(out.pair_units);
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.pair_offsets) {
        if (out.offsets64) static_cast<uint64_t*>(out.pair_offsets)[n_pairs] = pair_units;
        else static_cast<uint32_t*>(out.pair_offsets)[n_pairs] = static_cast<uint32_t>(pair_units);
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        if (valid && out.key_pairs && kflags[i] != 0) {
            const uint64_t jk = kidx_off[i];
            if (jk < n_keys) out.key_pairs[jk] = kpairs[slot_of[i]];
        }
        const bool first = valid && flags[i] != 0;
        uint64_t src = 0, dst = 0;
        uint32_t units = 0;
        if (first) {
            const uint64_t j = idx_off[i];
            const uint32_t pslot = pslot_of[i];
            dst = dst_off[i];
            if (j < n_pairs) {
                pairnum[pslot] = static_cast<uint32_t>(j);
                if (out.pair_key) out.pair_key[j] = keynum[slot_of[i]];
                if (out.pair_first_line) out.pair_first_line[j] = static_cast<uint32_t>(i);
                if (out.pair_lines) out.pair_lines[j] = pw[static_cast<uint64_t>(pslot) * GROUP_HEAD_WORDS + GROUP_W_LINES];
                if (out.pair_offsets) {
                    if (out.offsets64) static_cast<uint64_t*>(out.pair_offsets)[j] = dst;
                    else static_cast<uint32_t*>(out.pair_offsets)[j] = static_cast<uint32_t>(dst);
                }
                if (dst_units) {
                    uint32_t ks = 0;
                    const UNIT* p = batch.pair_of_line(static_cast<uint32_t>(i), ks, units);
                    units = plen[i];                                   // (the same number; the pass before kept it)
                    if (dst + units > pair_units) units = 0;           // (cannot be: the scan summed these very lengths)
                    src = static_cast<uint64_t>(p - data);
                }
            }
        }
        // the wave copies its first lines' seconds one after the other, 64 units a step: reads [src, src + units), writes [dst, dst + units)
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

__global__ void __launch_bounds__(256) k_pairs_line_pair(uint64_t n, const uint32_t* __restrict__ pslot_of, const uint32_t* __restrict__ pairnum,
                                                         uint32_t* __restrict__ line_pair) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t pslot = pslot_of[i];
        line_pair[i] = pslot == GROUP_NONE ? GROUP_NONE : pairnum[pslot];
    }
}

template <typename OFF, typename UNIT>
void launch_build_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const GroupArgs& a, const void* pairs_image, const GroupWs& g, const PairsWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *pi = static_cast<const uint4*>(pairs_image);
    u64 *table = reinterpret_cast<u64*>(w.table), *pw = reinterpret_cast<u64*>(w.head_words), *totals = reinterpret_cast<u64*>(w.totals);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_pairs_build<OFF, ROWS_U8, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           table, w.n_slots, pw, w.pslot_of, w.plen, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_pairs_build<OFF, ROWS_U16, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           table, w.n_slots, pw, w.pslot_of, w.plen, totals);
    else
        hipLaunchKernelGGL((k_pairs_build<OFF, ROWS_DENSE, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           table, w.n_slots, pw, w.pslot_of, w.plen, totals);
}

template <typename OFF, typename UNIT>
void launch_emit_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                    const GroupArgs& a, const void* pairs_image, const GroupWs& g, const PairsWs& w, const PairsOut& out, uint64_t n_pairs, uint64_t pair_units,
                    uint64_t n_keys) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *pi = static_cast<const uint4*>(pairs_image);
    const u64 *pw = reinterpret_cast<const u64*>(w.head_words), *kp = reinterpret_cast<const u64*>(w.kpairs);
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead) + sizeof(PairsHead));
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_pairs_emit<OFF, ROWS_U8, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           g.flags, g.idx_off, g.keynum, w.flags, w.pslot_of, w.plen, w.idx_off, w.dst_off, pw, kp, w.pairnum, out, n_pairs, pair_units, n_keys);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_pairs_emit<OFF, ROWS_U16, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           g.flags, g.idx_off, g.keynum, w.flags, w.pslot_of, w.plen, w.idx_off, w.dst_off, pw, kp, w.pairnum, out, n_pairs, pair_units, n_keys);
    else
        hipLaunchKernelGGL((k_pairs_emit<OFF, ROWS_DENSE, UNIT>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, pi, g.slot_of,
                           g.flags, g.idx_off, g.keynum, w.flags, w.pslot_of, w.plen, w.idx_off, w.dst_off, pw, kp, w.pairnum, out, n_pairs, pair_units, n_keys);
}

unsigned pairs_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048)); }   // (the build's grid)

size_t up16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

}  // namespace

// The pair slots' words, the key slots' pair counts and the totals -- zeroed before every call by ONE memset -- and the per-pair-slot
// pair numbers: [table n_slots][head 2 n_slots][kpairs n_key_slots][totals 8], all 64-bit, then pairnum[n_slots].
size_t pairs_table_zero_bytes(uint32_t n_slots, uint32_t n_key_slots) {
    return (static_cast<size_t>(n_slots) * (1u + GROUP_HEAD_WORDS) + static_cast<size_t>(n_key_slots) + 8u) * 8u;
}
size_t pairs_table_bytes(uint32_t n_slots, uint32_t n_key_slots) { return pairs_table_zero_bytes(n_slots, n_key_slots) + static_cast<size_t>(n_slots) * 4u; }

// The per-line arrays: idx_off and dst_off (n + 1, 64-bit), the two scans' block sums, pslot_of and plen (32-bit), flags.
size_t pairs_lines_bytes(uint64_t n) {
    return 2 * up16((n + 1) * 8) + 2 * scan_sums_bytes(n) + 2 * up16(n * 4) + up16(n);
}

PairsWs pairs_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, uint32_t n_key_slots) {
    PairsWs w{};
    w.n_slots = n_slots;
    w.n_key_slots = n_key_slots;
    uint64_t* t = static_cast<uint64_t*>(table_mem);
    w.table = t;
    w.head_words = t + n_slots;
    w.kpairs = w.head_words + static_cast<size_t>(n_slots) * GROUP_HEAD_WORDS;
    w.totals = w.kpairs + n_key_slots;
    w.pairnum = reinterpret_cast<uint32_t*>(w.totals + 8);
    uint8_t* p = static_cast<uint8_t*>(lines_mem);
    w.idx_off = reinterpret_cast<uint64_t*>(p); p += up16((n + 1) * 8);
    w.dst_off = reinterpret_cast<uint64_t*>(p); p += up16((n + 1) * 8);
    w.sums_a = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n);
    w.sums_b = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n);
    w.pslot_of = reinterpret_cast<uint32_t*>(p); p += up16(n * 4);
    w.plen = reinterpret_cast<uint32_t*>(p); p += up16(n * 4);
    w.flags = p;
    return w;
}

// Passes 1 and 2 on `stream`, n > 0 and parts > 0, behind launch_group_build: leaves w.totals (PairsDev), w.idx_off[n] = the pairs and
// w.dst_off[n] = their seconds' units.
hipError_t launch_pairs_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                              const void* pairs_image, const GroupWs& g, const PairsWs& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.table, 0, pairs_table_zero_bytes(w.n_slots, w.n_key_slots), stream);
    if (e != hipSuccess) return e;
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead) + sizeof(PairsHead)) + GROUP_LDS_ENTRIES * 4u + 16u + 32u + GROUP_LDS_ENTRIES * GROUP_HEAD_WORDS * 8u;
    const unsigned blocks = pairs_blocks(n);
    if (a.wide) {
        if (offsets64) launch_build_as<uint64_t, uint16_t>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w);
        else launch_build_as<uint32_t, uint16_t>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w);
    } else {
        if (offsets64) launch_build_as<uint64_t, uint8_t>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w);
        else launch_build_as<uint32_t, uint8_t>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pairs_flags, dim3(blocks), dim3(256), 0, stream, n, g.slot_of, w.pslot_of, reinterpret_cast<const u64*>(w.head_words), w.flags, w.plen,
                       reinterpret_cast<u64*>(w.kpairs));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(w.flags, n, w.sums_a, w.idx_off, stream);
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.plen, n, w.sums_b, w.dst_off, stream);
}

// Pass 3 on `stream`, behind launch_pairs_build, launch_group_emit and the host's check of the capacities.
hipError_t launch_pairs_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                             const void* pairs_image, const GroupWs& g, const PairsWs& w, const PairsOut& out, uint64_t n_pairs, uint64_t pair_units,
                             uint64_t n_keys, hipStream_t stream) {
    const unsigned blocks = pairs_blocks(n);
    if (a.wide) {
        if (offsets64) launch_emit_as<uint64_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w, out, n_pairs, pair_units, n_keys);
        else launch_emit_as<uint32_t, uint16_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w, out, n_pairs, pair_units, n_keys);
    } else {
        if (offsets64) launch_emit_as<uint64_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w, out, n_pairs, pair_units, n_keys);
        else launch_emit_as<uint32_t, uint8_t>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, pairs_image, g, w, out, n_pairs, pair_units, n_keys);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out.line_pair) return e;
    hipLaunchKernelGGL(k_pairs_line_pair, dim3(blocks), dim3(256), 0, stream, n, w.pslot_of, w.pairnum, out.line_pair);
    return hipGetLastError();
}

}  // namespace gx
