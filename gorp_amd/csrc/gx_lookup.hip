// gx_lookup.hip -- the passes of gx_lookup_lines / gx_text_lookup_lines: what the lines of a finished batch captured, looked up in a
// dictionary of texts the caller supplies, on the device.  The reference's caller does this right behind the extraction
// (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null && wanted.contains(r.asMap().get("user"))) ...     meta = byHost.get(r.asMap().get("host"));
// The rule -- slot word, lowest-entry word, find-only probe, classes -- is gx_lookup.hpp's; hash, table and find-or-insert are
// gx_group.hpp's; "a line counts" is gx_capture_stats' (gx_where_dev.hpp).
//
// 1. k_lookup_build: one lane per ENTRY, grid-stride.  hash -> group_find_or_insert as it stands (a 64-bit compare-and-swap on the table in
//    global memory; `same` reads the representative entry's units from the dictionary) -> an atomic maximum of the complemented entry
//    number into the slot's lowest-entry word -> slot_of_entry[j].  Which duplicate claimed a slot depends on timing; everything delivered
//    comes from the lowest-entry word.  An entry of 4 G units (or offsets that go backwards) sets a status bit and is not read.
// 2. k_lookup_probe, the hot path: one lane per line, k_group_build's grid.  outcome -> part -> terms -> key pair -> hash -> lookup_find.
//    The table is read-only here: plain loads.  What a hit ADDS to its slot -- one line, the minimum of the line number, and with a value
//    group StatsAcc's words -- is merged as k_group_build merges it: per distinct slot among the wave's 64 lines by ballot (a butterfly
//    only where a slot has several lines), then in the workgroup's LDS table (group_lds_entry, GroupAdd, group_add of gx_group_dev.hpp),
//    flushed once; a slot that finds the LDS table full adds to global memory.  The line's slot, LOOKUP_MISS or LOOKUP_NONE goes to
//    line_slot[i]; with keep the kept flag and the kept length go to the select workspace; lines, unset, hits and misses are summed per
//    wave, then per workgroup.
//    k_lookup_count, behind it and before the host's wait: distinct entries and those of them with a line, by ballot.
// 3. k_lookup_emit: per entry j, entry_same[j] from its slot's lowest-entry word; where that is j the slot's lines, first line and stats,
//    else zeros, 0xFFFFFFFF and the stats of nothing.  k_lookup_line_entry maps line_slot through the lowest-entry words.
// 4. With keep: gx_select.hip's two scans and its copy, as they are.
// Workspace, on the handle until gx_destroy: group_slots(m) slots -- two to four per entry, 64 at least -- of 32 bytes, 96 with a value
// group, so 64 .. 128 bytes per entry (192 .. 384); 4 more per entry; 4 per line; with keep gx_select_lines' workspace, 21 per line.
// DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_dev.hpp"
#include "gx_lookup.hpp"
#include "gx_outcome.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t lookup_smem[];

typedef unsigned long long u64;

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// the dictionary as the kernels read it: its offsets are 32 or 64 bits wide whatever the batch's are (the text form's batch has 32-bit ones)
template <typename UNIT>
struct DictDev {
    const UNIT* units;
    const void* off;
    int off64;
    __device__ __forceinline__ uint64_t at(uint64_t j) const {
        return off64 ? static_cast<const uint64_t*>(off)[j] : static_cast<uint64_t>(static_cast<const uint32_t*>(off)[j]);
    }
};

// the table while it is built: the policy of group_find_or_insert on the device (gx_group.hip's)
struct BuildTable {
    u64* words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t claim(uint32_t slot, uint64_t word) { return atomicCAS(words + slot, 0ull, static_cast<u64>(word)); }
};
// the finished table: plain loads
struct ProbeTable {
    const u64* __restrict__ words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return words[slot]; }
};

unsigned lookup_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048)); }

template <typename UNIT>
__global__ void __launch_bounds__(256) k_lookup_build(DictDev<UNIT> d, uint64_t m, uint32_t weak, u64* __restrict__ table, uint32_t n_slots, u64* __restrict__ low,
                                                      uint32_t* __restrict__ slot_of_entry, u64* __restrict__ totals) {
    BuildTable tab{table};
    uint32_t status = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < m; j += stride) {
        const uint64_t o0 = d.at(j), len = d.at(j + 1) - o0;
        uint32_t slot = GROUP_NONE;
        if (len > 0xFFFFFFFFull) {
            status |= 1u;   // (an entry of 4 G code units, or offsets that go backwards: refused by the host; its units are not read)
        } else {
            const UNIT* ep = d.units + o0;
            const uint32_t en = static_cast<uint32_t>(len), me = static_cast<uint32_t>(j);
            slot = group_find_or_insert(tab, n_slots, group_hash(ep, en, weak != 0u), me, ep, en, [&](uint32_t rep, const UNIT* a, uint32_t an) {
                if (rep == me) return true;
                const uint64_t b0 = d.at(rep);   // (rep is in the table: its length passed the test above)
                return group_same_key(a, an, d.units + b0, static_cast<uint32_t>(d.at(static_cast<uint64_t>(rep) + 1u) - b0));
            });
            if (slot == GROUP_NONE) status |= 2u;   // (cannot be: the table has two slots per entry)
            else atomicMax(low + slot, static_cast<u64>(lookup_low_word(me)));
        }
        slot_of_entry[j] = slot;
    }
    if (status) atomicOr(totals + 2, static_cast<u64>(status));
}

// LDS: GroupHead, the term image (wimage_bytes, 0: no terms), then keys[GROUP_LDS_ENTRIES], 4 words (used, spare), 8 totals (64-bit), and
// GROUP_LDS_ENTRIES x (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) 64-bit words.
// totals: 0 lines that count, 1 lines whose key pair names no value, 2 status bits, 3 hits, 4 misses.
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_lookup_probe(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                      uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                      const uint4* __restrict__ wimage, uint32_t wimage_bytes, DictDev<UNIT> d, const u64* __restrict__ table,
                                                      uint32_t n_slots, u64* __restrict__ gw, u64* __restrict__ gs, uint32_t* __restrict__ line_slot, uint32_t keep,
                                                      uint8_t* __restrict__ kflags, uint32_t* __restrict__ klen, u64* __restrict__ totals) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(lookup_smem);
    uint4* g_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    uint4* w_l = reinterpret_cast<uint4*>(smem + sizeof(GroupHead));
    for (uint32_t q = threadIdx.x; q < (wimage_bytes >> 4); q += 256u) w_l[q] = wimage[q];
    uint32_t* l_keys = reinterpret_cast<uint32_t*>(smem + sizeof(GroupHead) + wimage_bytes);
    uint32_t* l_used = l_keys + GROUP_LDS_ENTRIES;
    u64* l_totals = reinterpret_cast<u64*>(l_used + 4);
    u64* l_words = l_totals + 8;
    constexpr uint32_t EW = GROUP_HEAD_WORDS + GROUP_STATS_WORDS;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += 256u) l_keys[q] = GROUP_NONE;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES * EW; q += 256u) l_words[q] = 0ull;
    if (threadIdx.x < 4u) l_used[threadIdx.x] = 0u;
    if (threadIdx.x < 8u) l_totals[threadIdx.x] = 0ull;
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(smem);
    const WhereHead* wh = reinterpret_cast<const WhereHead*>(smem + sizeof(GroupHead));
    const UNIT* lits = reinterpret_cast<const UNIT*>(smem + sizeof(GroupHead) + sizeof(WhereHead));
    const uint32_t n_ext = gh->n_parts;
    const bool weak = (gh->flags & GROUP_WEAK_HASH) != 0u, values = gh->has_values != 0u;
    const uint32_t ext_lo = n_ext ? gh->ext[0] : 1u, ext_hi = n_ext ? gh->ext[n_ext - 1u] : 0u;
    const bool terms = wimage_bytes != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const ProbeTable tab{table};
    uint64_t t_lines = 0, t_unset = 0, t_hits = 0, t_misses = 0;   // (the same in every lane of the wave)
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
        uint32_t slot = LOOKUP_NONE;
        uint32_t cls = 3u;   // 0: a number, 1: unset, 2: no number, 3: the line has no value to measure
        int64_t v = 0;
        bool key_set = false;
        if (e < n_ext) {
            const GroupPart part = gh->part[e];
            int32_t pb, pe;
            pair_of<F>(ids, caps, i, row_units, slots, part.key_group, pb, pe);
            if (where_pair_set(pb, pe, line_units)) {
                key_set = true;
                const UNIT* kp = data + o0 + static_cast<uint32_t>(pb);
                const uint32_t kn = static_cast<uint32_t>(pe - pb);
                slot = lookup_find(tab, n_slots, group_hash(kp, kn, weak), kp, kn, [&](uint32_t rep, const UNIT* a, uint32_t an) {
                    const uint64_t b0 = d.at(rep);
                    return group_same_key(a, an, d.units + b0, static_cast<uint32_t>(d.at(static_cast<uint64_t>(rep) + 1u) - b0));
                });
                if (slot != LOOKUP_MISS && part.value_group != GROUP_NO_VALUE) {
                    pair_of<F>(ids, caps, i, row_units, slots, part.value_group, pb, pe);
                    if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                    else cls = number_parse_packed<NUM>(NUM ? gh->fmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                }
            }
        }
        const uint32_t what = lookup_class(e < n_ext, key_set, slot);
        if (valid) {
            line_slot[i] = slot;
            if (keep) {
                const bool kept = lookup_keeps(keep, what);
                kflags[i] = kept ? 1 : 0;
                klen[i] = kept ? static_cast<uint32_t>(line_units) : 0u;
            }
        }
        const bool hit = what == LOOKUP_HIT;
        t_lines += static_cast<uint64_t>(__popcll(__ballot(what != LOOKUP_SKIPPED)));
        t_unset += static_cast<uint64_t>(__popcll(__ballot(what == LOOKUP_UNSET)));
        t_misses += static_cast<uint64_t>(__popcll(__ballot(what == LOOKUP_IS_MISS)));
        // the distinct slots among the wave's 64 lines: every slot's lowest lane gathers what its lines add
        GroupAdd add{};
        bool leader = false;
        uint64_t todo = __ballot(hit);
        t_hits += static_cast<uint64_t>(__popcll(todo));
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint32_t ws = static_cast<uint32_t>(__shfl(static_cast<int>(slot), static_cast<int>(l)));
            const bool mine = hit && slot == ws;
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
                    for (int dd = 32; dd >= 1; dd >>= 1) {
                        lo += wave_xor64(lo, dd);
                        hi += wave_xor64(hi, dd);
                        mn = umax64(mn, wave_xor64(mn, dd));
                        mx = umax64(mx, wave_xor64(mx, dd));
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
            const uint32_t ent = group_lds_entry(l_keys, l_used, slot);
            if (ent != GROUP_NONE) {
                u64* w = l_words + ent * EW;
                group_add(w, w + GROUP_HEAD_WORDS, values, add);
            } else {
                group_add(gw + static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS, gs + static_cast<uint64_t>(slot) * GROUP_STATS_WORDS, values, add);
            }
        }
    }
    if (lane == 0u) {
        if (t_lines) atomicAdd(l_totals + 0, static_cast<u64>(t_lines));
        if (t_unset) atomicAdd(l_totals + 1, static_cast<u64>(t_unset));
        if (t_hits) atomicAdd(l_totals + 3, static_cast<u64>(t_hits));
        if (t_misses) atomicAdd(l_totals + 4, static_cast<u64>(t_misses));
    }
    // (status: every lane has its own bits)
    const uint64_t any1 = __ballot((t_status & 1u) != 0u);
    if (lane == 0u && any1) atomicOr(l_totals + 2, static_cast<u64>(1u));
    __syncthreads();
    if (threadIdx.x < 5u && l_totals[threadIdx.x]) {
        if (threadIdx.x == 2u) atomicOr(totals + 2, l_totals[2]);
        else atomicAdd(totals + threadIdx.x, l_totals[threadIdx.x]);
    }
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
}

// totals[5] += entries that are the lowest with their text; totals[6] += those of them that a line hit
__global__ void __launch_bounds__(256) k_lookup_count(uint64_t m, const uint32_t* __restrict__ slot_of_entry, const u64* __restrict__ low, const u64* __restrict__ gw,
                                                      u64* __restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t distinct = 0, hit = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); j0 < m; j0 += stride) {
        const uint64_t j = j0 + lane;
        bool is_low = false, has = false;
        if (j < m) {
            const uint32_t slot = slot_of_entry[j];
            if (slot != GROUP_NONE) {
                is_low = lookup_low_entry(low[slot]) == static_cast<uint32_t>(j);
                has = is_low && gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_LINES] != 0ull;
            }
        }
        distinct += static_cast<uint64_t>(__popcll(__ballot(is_low)));
        hit += static_cast<uint64_t>(__popcll(__ballot(has)));
    }
    if (lane == 0u) {
        if (distinct) atomicAdd(totals + 5, static_cast<u64>(distinct));
        if (hit) atomicAdd(totals + 6, static_cast<u64>(hit));
    }
}

// Per entry: the lowest entry with its text, and on that one what its slot gathered.
__global__ void __launch_bounds__(256) k_lookup_emit(uint64_t m, uint32_t values, const uint32_t* __restrict__ slot_of_entry, const u64* __restrict__ low,
                                                     const u64* __restrict__ gw, const u64* __restrict__ gs, LookupOut out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < m; j += stride) {
        const uint32_t slot = slot_of_entry[j];
        const uint32_t same = slot == GROUP_NONE ? static_cast<uint32_t>(j) : lookup_low_entry(low[slot]);   // (NONE: refused by the host before this runs)
        const bool mine = slot != GROUP_NONE && same == static_cast<uint32_t>(j);
        if (out.entry_same) out.entry_same[j] = same;
        uint64_t lines = 0, first = 0;
        if (mine) {
            lines = gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_LINES];
            first = gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_FIRST];
        }
        if (out.entry_lines) out.entry_lines[j] = lines;
        if (out.entry_first_line) out.entry_first_line[j] = first ? group_first_line(first) : 0xFFFFFFFFu;
        if (out.entry_stats) {
            uint64_t w[GROUP_STATS_WORDS], s[8];
#pragma unroll
            for (uint32_t q = 0; q < GROUP_STATS_WORDS; ++q) w[q] = (mine && values) ? gs[static_cast<uint64_t>(slot) * GROUP_STATS_WORDS + q] : 0ull;
            group_stats_out(w, s);
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) out.entry_stats[j * 8u + q] = s[q];
        }
    }
}

__global__ void __launch_bounds__(256) k_lookup_line_entry(uint64_t n, const uint32_t* __restrict__ line_slot, const u64* __restrict__ low,
                                                           uint32_t* __restrict__ line_entry) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = line_slot[i];
        line_entry[i] = slot >= LOOKUP_MISS ? slot : lookup_low_entry(low[slot]);
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_probe_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const GroupArgs& a, const LookupDict& dict, uint32_t keep, const LookupWs& w, const SelectWs* sel) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* dt = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *wi = static_cast<const uint4*>(a.where_image);
    const DictDev<UNIT> d{static_cast<const UNIT*>(dict.units), dict.offsets, dict.offsets64};
    const u64* table = reinterpret_cast<const u64*>(w.table);
    u64 *gw = reinterpret_cast<u64*>(w.head_words), *gs = reinterpret_cast<u64*>(w.stats_words), *totals = reinterpret_cast<u64*>(w.totals);
    uint8_t* kf = sel ? sel->flags : nullptr;
    uint32_t* kl = sel ? sel->klen : nullptr;
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_lookup_probe<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, dt, gi, wi,
                           a.where_image_bytes, d, table, w.n_slots, gw, gs, w.line_slot, keep, kf, kl, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_lookup_probe<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, dt, gi, wi,
                           a.where_image_bytes, d, table, w.n_slots, gw, gs, w.line_slot, keep, kf, kl, totals);
    else
        hipLaunchKernelGGL((k_lookup_probe<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, dt, gi, wi,
                           a.where_image_bytes, d, table, w.n_slots, gw, gs, w.line_slot, keep, kf, kl, totals);
}

size_t up16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

}  // namespace

// The slots' words, zeroed before every call by ONE memset: [table n_slots][low n_slots][head 2 n_slots][stats 8 n_slots, with values]
// [totals 8], all 64-bit.
size_t lookup_table_zero_bytes(uint32_t n_slots, bool values) {
    return (static_cast<size_t>(n_slots) * (2u + GROUP_HEAD_WORDS + (values ? GROUP_STATS_WORDS : 0u)) + 8u) * 8u;
}
size_t lookup_table_bytes(uint32_t n_slots, bool values) { return lookup_table_zero_bytes(n_slots, values); }
// slot_of_entry[m] and line_slot[n], 32-bit
size_t lookup_lines_bytes(uint64_t n, uint64_t m) { return up16(m * 4) + up16(n * 4) + 16; }

LookupWs lookup_workspace(void* table_mem, void* lines_mem, uint64_t n, uint64_t m, uint32_t n_slots, bool values) {
    LookupWs w{};
    w.n_slots = n_slots;
    uint64_t* t = static_cast<uint64_t*>(table_mem);
    w.table = t;
    w.low = t + n_slots;
    w.head_words = w.low + n_slots;
    w.stats_words = w.head_words + static_cast<size_t>(n_slots) * GROUP_HEAD_WORDS;   // (never touched without values)
    w.totals = w.stats_words + (values ? static_cast<size_t>(n_slots) * GROUP_STATS_WORDS : 0u);
    uint8_t* p = static_cast<uint8_t*>(lines_mem);
    w.slot_of_entry = reinterpret_cast<uint32_t*>(p); p += up16(m * 4);
    w.line_slot = reinterpret_cast<uint32_t*>(p);
    (void)n;
    return w;
}

hipError_t launch_lookup_probe(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const LookupDict& d, uint32_t keep, const LookupWs& w, const SelectWs* sel, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.table, 0, lookup_table_zero_bytes(w.n_slots, a.has_values != 0), stream);
    if (e != hipSuccess) return e;
    if (keep && !sel) return hipErrorInvalidValue;
    u64 *table = reinterpret_cast<u64*>(w.table), *low = reinterpret_cast<u64*>(w.low), *totals = reinterpret_cast<u64*>(w.totals);
    if (d.m) {
        const unsigned blocks = lookup_blocks(d.m);
        if (a.wide)
            hipLaunchKernelGGL(k_lookup_build<uint16_t>, dim3(blocks), dim3(256), 0, stream, DictDev<uint16_t>{static_cast<const uint16_t*>(d.units), d.offsets, d.offsets64},
                               d.m, d.weak_hash, table, w.n_slots, low, w.slot_of_entry, totals);
        else
            hipLaunchKernelGGL(k_lookup_build<uint8_t>, dim3(blocks), dim3(256), 0, stream, DictDev<uint8_t>{static_cast<const uint8_t*>(d.units), d.offsets, d.offsets64},
                               d.m, d.weak_hash, table, w.n_slots, low, w.slot_of_entry, totals);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n) {
        const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead)) + a.where_image_bytes + GROUP_LDS_ENTRIES * 4u + 16u + 64u +
                             GROUP_LDS_ENTRIES * (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) * 8u;
        if (lds > 64u * 1024u) return hipErrorInvalidValue;   // (64 terms of 255 two-byte units: 34 KiB; GroupHead and the LDS table: 11.1 KiB)
        const unsigned blocks = lookup_blocks(n);
        auto go = [&](auto off_t, auto unit_t) {
            using OFF = decltype(off_t);
            using UNIT = decltype(unit_t);
            if (a.formats) launch_probe_as<OFF, UNIT, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, d, keep, w, sel);
            else launch_probe_as<OFF, UNIT, false>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, d, keep, w, sel);
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
    }
    if (d.m) {
        hipLaunchKernelGGL(k_lookup_count, dim3(lookup_blocks(d.m)), dim3(256), 0, stream, d.m, w.slot_of_entry, low, reinterpret_cast<const u64*>(w.head_words), totals);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_lookup_emit(uint64_t n, uint64_t m, bool values, const LookupWs& w, const LookupOut& out, hipStream_t stream) {
    const u64 *low = reinterpret_cast<const u64*>(w.low), *gw = reinterpret_cast<const u64*>(w.head_words), *gs = reinterpret_cast<const u64*>(w.stats_words);
    if (m && (out.entry_same || out.entry_lines || out.entry_first_line || out.entry_stats)) {
        hipLaunchKernelGGL(k_lookup_emit, dim3(lookup_blocks(m)), dim3(256), 0, stream, m, values ? 1u : 0u, w.slot_of_entry, low, gw, gs, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n && out.line_entry) {
        hipLaunchKernelGGL(k_lookup_line_entry, dim3(lookup_blocks(n)), dim3(256), 0, stream, n, w.line_slot, low, out.line_entry);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace gx
