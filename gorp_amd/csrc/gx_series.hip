// gx_series.hip -- the passes of gx_group_series / gx_text_group_series: the lines of a finished batch counted and measured per (captured
// text, interval of a captured number), on the device.  The reference's caller does this right behind the extraction (README.md:26,63-79,
// with a timestamp field):
//     long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
//     perVerb.computeIfAbsent(r.asMap().get("verb"), v -> new TreeMap<Long, Stats>()).computeIfAbsent(b, x -> new Stats()).record(...);
// The rule -- the classes of a keyed line, cell_word, sort_word, the digit plans -- is gx_series.hpp's; what one cell slot receives and
// the workgroup's LDS table are gx_group_dev.hpp's (GroupAdd, group_add, group_lds_entry: this file is their third user, beside
// gx_group.hip and gx_bucket.hip); the flags, compact, count and scatter kernels are gx_bucket_sort_dev.hpp's.  All passes run behind
// launch_group_build (gx_group.hip), which leaves slot_of[] complete and is not changed: a line's key IS its key slot.
//
// 1. k_series_build: one lane per line, grid-stride, k_bucket_build's grid and instantiations.  Lines without a key slot are skipped; the
//    others count and are keyed, so no term is evaluated again.  outcome -> part -> number pair -> parse -> bucket -> word.  The wave
//    FIRST finds its distinct bucket words by ballot (time-ordered logs: one or two rounds); only each word's lowest lane goes to the
//    bucket table in global memory and hands the bucket slot to its lines by shuffle.  Then the wave finds its distinct cell words
//    (cell_word(key slot, bucket slot)) the same way; each cell's lowest lane gathers what its lines add (a butterfly only where several
//    lines carry numbers), and ONLY that lane goes to the cell table.  What it gathered goes to the workgroup's LDS table
//    (group_lds_entry, keyed by cell slot), flushed once; a workgroup that meets more cells than that table claims adds the surplus to
//    global memory directly.  The line's cell slot goes to cslot_of[i].  All merges are unsigned adds and maxima of 64-bit integers.
// 2. k_bucket_flags + a scan (gx_scan.hpp) over each table's slots: [n_slots] = the buckets and the cells, read by the host in the one
//    wait in which it reads gx_group_lines' totals and SeriesDev.
// Behind that wait and behind launch_group_emit, which numbers the key slots:
// 3. the buckets' (word, bucket slot) pairs, compacted and sorted over bucket_digits(min, max) digits (gx_bucket_sort_dev.hpp);
//    k_series_axis writes bucket_number[] and rank_of_bslot[].
// 4. k_series_cells compacts the cells into (sort_word(keynum[key slot], rank_of_bslot[bucket slot]), cell slot) pairs; the same sort over
//    series_digits(n_keys, n_buckets) digits.
// 5. k_series_emit: one lane per rank c: cell_key, cell_bucket, cell_first_line, cell_lines, cell_stats, rank_of_cslot[]; k_series_bounds:
//    key_cell_begin[j] by lower bound over the sorted key numbers (gx_by_key.hpp's rule: a key without a cell has an empty run);
//    k_series_line: line_cell[i] = rank_of_cslot[cslot_of[i]].
// No workgroup waits for another, every loop is bounded by an argument or a constant.  DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_bucket.hpp"
#include "gx_bucket_sort_dev.hpp"
#include "gx_by_key.hpp"
#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_dev.hpp"
#include "gx_outcome.hpp"
#include "gx_radix_dev.hpp"
#include "gx_scan.hpp"
#include "gx_series.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t series_smem[];

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// a one-word table in global memory: the policy of bucket_find_or_insert on the device
struct SeriesDevTable {
    u64* words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t claim(uint32_t slot, uint64_t word) { return atomicCAS(words + slot, 0ull, static_cast<u64>(word)); }
};

// LDS: GroupHead, SeriesHead, then keys[GROUP_LDS_ENTRIES], 4 words (used, spare), 8 totals (SeriesDev's fields), and GROUP_LDS_ENTRIES x
// (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) 64-bit words.
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(BUCKET_WG_LINES) k_series_build(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                      uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                      const uint4* __restrict__ simage, const uint32_t* __restrict__ slot_of, u64* __restrict__ btable,
                                                      u64* __restrict__ ctable, uint32_t n_slots, u64* __restrict__ cw, u64* __restrict__ cs,
                                                      uint32_t* __restrict__ cslot_of, u64* __restrict__ totals) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(series_smem);
    uint4* g_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += BUCKET_WG_LINES) g_l[q] = gimage[q];
    uint4* s_l = reinterpret_cast<uint4*>(smem + sizeof(GroupHead));
    for (uint32_t q = threadIdx.x; q < (sizeof(SeriesHead) >> 4); q += BUCKET_WG_LINES) s_l[q] = simage[q];
    uint32_t* l_keys = reinterpret_cast<uint32_t*>(smem + sizeof(GroupHead) + sizeof(SeriesHead));
    uint32_t* l_used = l_keys + GROUP_LDS_ENTRIES;
    u64* l_totals = reinterpret_cast<u64*>(l_used + 4);
    u64* l_words = l_totals + 8;
    constexpr uint32_t EW = GROUP_HEAD_WORDS + GROUP_STATS_WORDS;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += BUCKET_WG_LINES) l_keys[q] = GROUP_NONE;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES * EW; q += BUCKET_WG_LINES) l_words[q] = 0ull;
    if (threadIdx.x < 4u) l_used[threadIdx.x] = 0u;
    if (threadIdx.x < 8u) l_totals[threadIdx.x] = 0ull;
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(smem);
    const SeriesHead* sh = reinterpret_cast<const SeriesHead*>(smem + sizeof(GroupHead));
    const uint32_t n_ext = gh->n_parts;
    const bool weak = (gh->flags & GROUP_WEAK_HASH) != 0u, values = gh->has_values != 0u;
    const int64_t origin = sh->origin;
    const uint64_t width = sh->width ? sh->width : 1u;   // (it is >= 1: the host refuses the rest)
    const uint32_t lane = threadIdx.x & 63u;
    SeriesDevTable btab{btable}, ctab{ctable};
    uint64_t t_celled = 0, t_unset = 0, t_nan = 0, t_oor = 0;   // (the same in every lane of the wave)
    bool t_full = false;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * BUCKET_WG_LINES;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * BUCKET_WG_LINES + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        const uint32_t kslot = valid ? slot_of[i] : GROUP_NONE;
        const bool keyed = kslot != GROUP_NONE;   // (the line counts and its key pair is set: the build found it so)
        uint64_t bword = 0;   // the line's bucket word; 0: it is not celled
        uint32_t why = 0u;    // of a keyed line that is not celled -- 1: number unset, 2: no number, 3: out of range
        uint32_t cls = 3u;    // the value -- 0: a number, 1: unset, 2: no number, 3: the line has no value to measure
        int64_t v = 0;
        if (keyed) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            const uint32_t e = where_find(gh->ext, n_ext, oc);
            const int32_t ng = e < n_ext ? sh->number[e] : SERIES_NO_NUMBER;   // (e < n_ext: a keyed line's outcome has a part)
            if (ng < 0) why = 1u;
            else {
                const uint64_t o0 = static_cast<uint64_t>(off[i]);
                const uint64_t line_units = static_cast<uint64_t>(off[i + 1]) - o0;   // (< 4 G: the build gives no key to a longer line)
                int32_t pb, pe;
                pair_of<F>(ids, caps, i, row_units, slots, static_cast<uint32_t>(ng), pb, pe);
                int64_t num = 0, b = 0;
                if (!where_pair_set(pb, pe, line_units)) why = 1u;
                else if (!number_parse_packed<NUM>(NUM ? sh->nfmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &num)) why = 2u;
                else if (!bucket_of(num, origin, width, &b)) why = 3u;
                else {
                    bword = bucket_word(b);
                    const GroupPart part = gh->part[e];
                    if (part.value_group != GROUP_NO_VALUE) {
                        pair_of<F>(ids, caps, i, row_units, slots, part.value_group, pb, pe);
                        if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                        else cls = number_parse_packed<NUM>(NUM ? gh->fmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                    }
                }
            }
        }
        t_celled += static_cast<uint64_t>(__popcll(__ballot(bword != 0ull)));
        t_unset += static_cast<uint64_t>(__popcll(__ballot(why == 1u)));
        t_nan += static_cast<uint64_t>(__popcll(__ballot(why == 2u)));
        t_oor += static_cast<uint64_t>(__popcll(__ballot(why == 3u)));
        // the distinct bucket words among the wave's 64 lines: every word's lowest lane leads its lines to the bucket table
        bool leader = false;
        uint32_t lead = lane;
        uint64_t todo = __ballot(bword != 0ull);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint64_t ww = static_cast<uint64_t>(__shfl(static_cast<u64>(bword), static_cast<int>(l)));
            const bool mine = bword == ww;   // (ww != 0: a lane without a bucket is nobody's)
            if (mine) lead = l;
            if (lane == l) leader = true;
            todo &= ~__ballot(mine);
        }
        uint32_t bslot = GROUP_NONE;
        if (leader) {
            bslot = bucket_find_or_insert(btab, n_slots, bword, weak);
            if (bslot == GROUP_NONE) t_full = true;
            else {
                atomicMax(l_totals + 5, static_cast<u64>(~bword));
                atomicMax(l_totals + 6, static_cast<u64>(bword));
            }
        }
        bslot = static_cast<uint32_t>(__shfl(static_cast<int>(bslot), static_cast<int>(lead)));   // (a lane without a bucket leads itself: GROUP_NONE)
        // the distinct cell words: every word's lowest lane gathers what its lines add, and leads them to the cell table
        const uint64_t cword = bslot != GROUP_NONE ? cell_word(kslot, bslot) : 0ull;   // (bslot is a slot: the line is keyed and celled)
        GroupAdd add{};
        leader = false;
        lead = lane;
        todo = __ballot(cword != 0ull);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint64_t ww = static_cast<uint64_t>(__shfl(static_cast<u64>(cword), static_cast<int>(l)));
            const bool mine = cword == ww;
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
                if (numbers & (numbers - 1ull)) {                         // (several lines carry numbers: a butterfly; one line has its own)
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        lo += wave_xor64(lo, d);
                        hi += wave_xor64(hi, d);
                        mn = umax64(mn, wave_xor64(mn, d));
                        mx = umax64(mx, wave_xor64(mx, d));
                    }
                } else if (numbers) {                                     // (one line carries the number: the cell's lowest lane takes it from there)
                    const int from = __ffsll(static_cast<u64>(numbers)) - 1;
                    lo = static_cast<uint64_t>(__shfl(static_cast<u64>(lo), from));
                    hi = static_cast<uint64_t>(__shfl(static_cast<u64>(hi), from));
                    mn = static_cast<uint64_t>(__shfl(static_cast<u64>(mn), from));
                    mx = static_cast<uint64_t>(__shfl(static_cast<u64>(mx), from));
                }
            }
            if (mine) lead = l;
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
        uint32_t cslot = GROUP_NONE;
        if (leader) {
            cslot = bucket_find_or_insert(ctab, n_slots, cword, weak);
            if (cslot == GROUP_NONE) t_full = true;
        }
        cslot = static_cast<uint32_t>(__shfl(static_cast<int>(cslot), static_cast<int>(lead)));   // (a lane without a cell leads itself: GROUP_NONE)
        if (valid) cslot_of[i] = cslot;
        if (leader && cslot != GROUP_NONE) {
            const uint32_t ent = group_lds_entry(l_keys, l_used, cslot);
            if (ent != GROUP_NONE) {
                u64* w = l_words + ent * EW;
                group_add(w, w + GROUP_HEAD_WORDS, values, add);
            } else {
                group_add(cw + static_cast<uint64_t>(cslot) * GROUP_HEAD_WORDS, cs + static_cast<uint64_t>(cslot) * GROUP_STATS_WORDS, values, add);
            }
        }
    }
    if (lane == 0u) {
        if (t_celled) atomicAdd(l_totals + 0, static_cast<u64>(t_celled));
        if (t_unset) atomicAdd(l_totals + 1, static_cast<u64>(t_unset));
        if (t_nan) atomicAdd(l_totals + 2, static_cast<u64>(t_nan));
        if (t_oor) atomicAdd(l_totals + 3, static_cast<u64>(t_oor));
    }
    const uint64_t any_full = __ballot(t_full);   // (every lane has its own)
    if (lane == 0u && any_full) atomicOr(l_totals + 4, static_cast<u64>(2u));
    __syncthreads();
    if (threadIdx.x < 7u && l_totals[threadIdx.x]) {
        if (threadIdx.x == 4u) atomicOr(totals + 4, l_totals[4]);
        else if (threadIdx.x >= 5u) atomicMax(totals + threadIdx.x, l_totals[threadIdx.x]);
        else atomicAdd(totals + threadIdx.x, l_totals[threadIdx.x]);
    }
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += BUCKET_WG_LINES) {
        const uint32_t s = l_keys[q];
        if (s == GROUP_NONE) continue;
        const u64* w = l_words + q * EW;
        if (w[GROUP_W_LINES] == 0ull) continue;   // (claimed by a lane whose words went elsewhere: nothing to flush)
        const u64* st = w + GROUP_HEAD_WORDS;
        const GroupAdd a{w[GROUP_W_LINES], w[GROUP_W_FIRST], st[GROUP_S_NUMBERS], st[GROUP_S_UNSET], st[GROUP_S_NOT_NUMBERS], st[GROUP_S_MIN], st[GROUP_S_MAX],
                          st[GROUP_S_LO], st[GROUP_S_HI]};
        group_add(cw + static_cast<uint64_t>(s) * GROUP_HEAD_WORDS, cs + static_cast<uint64_t>(s) * GROUP_STATS_WORDS, values, a);
    }
}

// One lane per rank j of the sorted bucket words: the axis and the bucket slot's rank.  m <= bucket_number's capacity where it is given.
__global__ void __launch_bounds__(256) k_series_axis(const uint64_t* __restrict__ word, const uint32_t* __restrict__ slot, uint32_t m, uint32_t n_slots,
                                                     uint32_t* __restrict__ rank_of_bslot, int64_t* __restrict__ bucket_number_out) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t s = slot[j];
    if (s >= n_slots) return;   // (it is not: the compaction wrote slot numbers)
    rank_of_bslot[s] = static_cast<uint32_t>(j);
    if (bucket_number_out) bucket_number_out[j] = bucket_number(word[j]);
}

// word[at], slot[at] = the sort word of cell slot s's cell and s, at = the occupied cell slots before s; m: the cells the host read
__global__ void __launch_bounds__(256) k_series_cells(const u64* __restrict__ ctable, uint32_t n_slots, const uint8_t* __restrict__ occupied,
                                                      const uint64_t* __restrict__ before, uint32_t m, const uint32_t* __restrict__ keynum, uint32_t n_key_slots,
                                                      const uint32_t* __restrict__ rank_of_bslot, uint64_t n_buckets, uint64_t* __restrict__ word,
                                                      uint32_t* __restrict__ slot) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; s < n_slots; s += stride) {
        if (!occupied[s]) continue;
        const uint64_t at = before[s];
        if (at >= m) continue;   // (it is not: the scan counted these very flags, and the host read m from it)
        const uint64_t cw = ctable[s];
        const uint32_t kslot = cell_kslot(cw), bslot = cell_bslot(cw);
        if (kslot >= n_key_slots || bslot >= n_slots) continue;   // (they are not: the build made the word from a key slot and a bucket slot)
        word[at] = sort_word(keynum[kslot], rank_of_bslot[bslot], n_buckets);
        slot[at] = static_cast<uint32_t>(s);
    }
}

// One lane per rank c of the sorted cells: the cell's row, its key number for the bounds, its slot's rank.  m <= the per-cell arrays'
// capacity (the host has checked it).
__global__ void __launch_bounds__(256) k_series_emit(const uint64_t* __restrict__ word, const uint32_t* __restrict__ slot, uint32_t m, uint32_t n_slots,
                                                     uint64_t n_buckets, const u64* __restrict__ cw, const u64* __restrict__ cs, uint32_t* __restrict__ rank_of_cslot,
                                                     uint32_t* __restrict__ knum, SeriesOut out) {
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (c >= m) return;
    const uint32_t s = slot[c];
    if (s >= n_slots) return;   // (it is not: the compaction wrote slot numbers)
    const uint64_t w = word[c];
    const uint32_t key = static_cast<uint32_t>(w / n_buckets), rank = static_cast<uint32_t>(w % n_buckets);   // (n_buckets >= 1: there is a cell)
    rank_of_cslot[s] = static_cast<uint32_t>(c);
    knum[c] = key;
    if (out.cell_key) out.cell_key[c] = key;
    if (out.cell_bucket) out.cell_bucket[c] = rank;
    if (out.cell_first_line) out.cell_first_line[c] = group_first_line(cw[static_cast<uint64_t>(s) * GROUP_HEAD_WORDS + GROUP_W_FIRST]);
    if (out.cell_lines) out.cell_lines[c] = cw[static_cast<uint64_t>(s) * GROUP_HEAD_WORDS + GROUP_W_LINES];
    if (out.cell_stats) {
        uint64_t sw[GROUP_STATS_WORDS], st[8];
#pragma unroll
        for (uint32_t q = 0; q < GROUP_STATS_WORDS; ++q) sw[q] = cs[static_cast<uint64_t>(s) * GROUP_STATS_WORDS + q];
        group_stats_out(sw, st);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) out.cell_stats[c * 8u + q] = st[q];
    }
}

// One lane per key j in 0 .. n_keys: where key j's cells begin among the m sorted cells; [n_keys] = m.
__global__ void __launch_bounds__(256) k_series_bounds(const uint32_t* __restrict__ knum, uint64_t m, uint64_t n_keys, uint64_t* __restrict__ key_cell_begin) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > n_keys) return;
    key_cell_begin[j] = by_key_begin(knum, m, j);
}

__global__ void __launch_bounds__(256) k_series_line(uint64_t n, const uint32_t* __restrict__ cslot_of, const uint32_t* __restrict__ rank_of_cslot, uint32_t n_slots,
                                                     uint32_t* __restrict__ line_cell) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = cslot_of[i];
        line_cell[i] = slot < n_slots ? rank_of_cslot[slot] : GROUP_NONE;
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_build_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const GroupArgs& a, const void* series_image, const GroupWs& g, const SeriesWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *si = static_cast<const uint4*>(series_image);
    u64 *bt = reinterpret_cast<u64*>(w.btable), *ct = reinterpret_cast<u64*>(w.ctable), *cw = reinterpret_cast<u64*>(w.head_words),
        *cs = reinterpret_cast<u64*>(w.stats_words), *totals = reinterpret_cast<u64*>(w.totals);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_series_build<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si,
                           g.slot_of, bt, ct, w.n_slots, cw, cs, w.cslot_of, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_series_build<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si,
                           g.slot_of, bt, ct, w.n_slots, cw, cs, w.cslot_of, totals);
    else
        hipLaunchKernelGGL((k_series_build<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si,
                           g.slot_of, bt, ct, w.n_slots, cw, cs, w.cslot_of, totals);
}

unsigned series_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048)); }   // (k_bucket_build's grid)
static_assert(BUCKET_WG_LINES == 256, "series_blocks gives the build pass one workgroup per 256 lines");
uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }

// the sort of the m pairs in s.word[0] / s.slot[0] over n_digits digits from the lowest; returns the buffer that holds the result
hipError_t sort_pairs(const BucketSortWs& s, uint32_t m32, uint32_t n_digits, hipStream_t stream, uint32_t* result) {
    const uint64_t blocks64 = sort_blocks(m32);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    uint32_t cur = 0;
    for (uint32_t d = 0; d < n_digits; ++d) {
        hipLaunchKernelGGL(k_bucket_count, dim3(blocks), dim3(256), 0, stream, s.word[cur], m32, d, s.slab);
        const hipError_t e = launch_exclusive_scan<uint32_t>(s.slab, 64u * blocks64, s.block_sums, s.bases, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bucket_scatter, dim3(blocks), dim3(256), 0, stream, s.word[cur], s.slot[cur], m32, d, s.bases, s.word[cur ^ 1u], s.slot[cur ^ 1u]);
        cur ^= 1u;
    }
    *result = cur;
    return hipGetLastError();
}

}  // namespace

// Both tables' words, the cells' per-slot words and the totals -- zeroed before every call by ONE memset: [buckets n_slots][cells n_slots]
// [head 2 n_slots][stats 8 n_slots, with values][totals 8], all 64-bit -- then per table before[n_slots + 1], the scan's sums, the ranks
// [n_slots] and occupied[n_slots]: 58 bytes per slot, 122 with values.
size_t series_table_zero_bytes(uint32_t n_slots, bool values) {
    return (static_cast<size_t>(n_slots) * (2u + GROUP_HEAD_WORDS + (values ? GROUP_STATS_WORDS : 0u)) + 8u) * 8u;
}
size_t series_table_bytes(uint32_t n_slots, bool values) {
    return series_table_zero_bytes(n_slots, values) +
           2u * (pad16((static_cast<uint64_t>(n_slots) + 1u) * 8u) + scan_sums_bytes(n_slots) + pad16(static_cast<uint64_t>(n_slots) * 4u) + pad16(n_slots));
}
// the per-line array: cslot_of (32-bit)
size_t series_lines_bytes(uint64_t n) { return pad16(n * 4u); }

SeriesWs series_workspace(void* table_mem, void* lines_mem, uint32_t n_slots, bool values) {
    SeriesWs w{};
    w.n_slots = n_slots;
    uint64_t* t = static_cast<uint64_t*>(table_mem);
    w.btable = t;
    w.ctable = t + n_slots;
    w.head_words = w.ctable + n_slots;
    w.stats_words = w.head_words + static_cast<size_t>(n_slots) * GROUP_HEAD_WORDS;   // (never touched without values)
    w.totals = w.stats_words + (values ? static_cast<size_t>(n_slots) * GROUP_STATS_WORDS : 0u);
    uint8_t* p = reinterpret_cast<uint8_t*>(w.totals + 8);
    w.bbefore = reinterpret_cast<uint64_t*>(p); p += pad16((static_cast<uint64_t>(n_slots) + 1u) * 8u);
    w.cbefore = reinterpret_cast<uint64_t*>(p); p += pad16((static_cast<uint64_t>(n_slots) + 1u) * 8u);
    w.bsums = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n_slots);
    w.csums = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n_slots);
    w.rank_of_bslot = reinterpret_cast<uint32_t*>(p); p += pad16(static_cast<uint64_t>(n_slots) * 4u);
    w.rank_of_cslot = reinterpret_cast<uint32_t*>(p); p += pad16(static_cast<uint64_t>(n_slots) * 4u);
    w.boccupied = p; p += pad16(n_slots);
    w.coccupied = p;
    w.cslot_of = static_cast<uint32_t*>(lines_mem);
    return w;
}

// The sorts' workspace for m cells (the buckets, no more than the cells, are sorted in it first): bucket_sort_workspace's 24 bytes per
// cell and 768 per 2 048 of them, and the sorted cells' key numbers (4 bytes per cell).
size_t series_sort_workspace_bytes(uint64_t m) { return bucket_sort_workspace_bytes(m) + pad16(m * 4u); }
SeriesSortWs series_sort_workspace(void* ws, uint64_t m) {
    SeriesSortWs s{};
    s.sort = bucket_sort_workspace(ws, m);
    s.knum = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + s.sort.bytes);
    return s;
}

// Passes 1 and 2 on `stream`, n > 0 and parts > 0, behind launch_group_build: leaves w.totals (SeriesDev), w.bbefore[n_slots] = the buckets
// and w.cbefore[n_slots] = the cells.  a.image (GroupHead) and series_image (SeriesHead) are on the device.
hipError_t launch_series_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const void* series_image, bool formats, const GroupWs& g, const SeriesWs& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.btable, 0, series_table_zero_bytes(w.n_slots, a.has_values != 0), stream);
    if (e != hipSuccess) return e;
    const uint32_t lds = static_cast<uint32_t>(sizeof(GroupHead) + sizeof(SeriesHead)) + GROUP_LDS_ENTRIES * 4u + 16u + 64u +
                         GROUP_LDS_ENTRIES * (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) * 8u;   // (11.8 KiB)
    const unsigned blocks = series_blocks(n);
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (formats) launch_build_as<OFF, UNIT, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, series_image, g, w);
        else launch_build_as<OFF, UNIT, false>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, series_image, g, w);
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
    const unsigned sblocks = series_blocks(w.n_slots);
    hipLaunchKernelGGL(k_bucket_flags, dim3(sblocks), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.btable), w.n_slots, w.boccupied);
    hipLaunchKernelGGL(k_bucket_flags, dim3(sblocks), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.ctable), w.n_slots, w.coccupied);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(w.boccupied, w.n_slots, w.bsums, w.bbefore, stream);
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint8_t>(w.coccupied, w.n_slots, w.csums, w.cbefore, stream);
}

// Passes 3, 4 and 5 on `stream`, behind launch_series_build, launch_group_emit (g.keynum) and the host's read of n_buckets =
// w.bbefore[n_slots], n_cells = w.cbefore[n_slots] (0 < n_buckets <= n_cells <= n_slots, each within its outputs' capacity), of the
// smallest and largest bucket word (b_digits) and of n_keys (c_digits: series_digits, or all of them).
hipError_t launch_series_emit(uint64_t n, uint64_t n_keys, uint64_t n_buckets, uint64_t n_cells, uint32_t b_digits, uint32_t c_digits, const GroupWs& g,
                              const SeriesWs& w, const SeriesSortWs& s, const SeriesOut& out, hipStream_t stream) {
    if (n_buckets == 0 || n_buckets > n_cells || n_cells > w.n_slots || b_digits > BUCKET_MAX_DIGITS || c_digits > BUCKET_MAX_DIGITS) return hipErrorInvalidValue;
    const uint32_t nb = static_cast<uint32_t>(n_buckets), nc = static_cast<uint32_t>(n_cells);
    const unsigned sblocks = series_blocks(w.n_slots);
    hipLaunchKernelGGL(k_bucket_compact, dim3(sblocks), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.btable), w.n_slots, w.boccupied, w.bbefore, nb,
                       s.sort.word[0], s.sort.slot[0]);
    uint32_t cur = 0;
    hipError_t e = sort_pairs(s.sort, nb, b_digits, stream, &cur);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_series_axis, dim3(static_cast<unsigned>((n_buckets + 255) / 256)), dim3(256), 0, stream, s.sort.word[cur], s.sort.slot[cur], nb, w.n_slots,
                       w.rank_of_bslot, out.bucket_number);
    hipLaunchKernelGGL(k_series_cells, dim3(sblocks), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.ctable), w.n_slots, w.coccupied, w.cbefore, nc, g.keynum,
                       g.n_slots, w.rank_of_bslot, n_buckets, s.sort.word[0], s.sort.slot[0]);
    e = sort_pairs(s.sort, nc, c_digits, stream, &cur);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_series_emit, dim3(static_cast<unsigned>((n_cells + 255) / 256)), dim3(256), 0, stream, s.sort.word[cur], s.sort.slot[cur], nc, w.n_slots,
                       n_buckets, reinterpret_cast<const u64*>(w.head_words), reinterpret_cast<const u64*>(w.stats_words), w.rank_of_cslot, s.knum, out);
    if (out.key_cell_begin)
        hipLaunchKernelGGL(k_series_bounds, dim3(static_cast<unsigned>((n_keys + 1 + 255) / 256)), dim3(256), 0, stream, s.knum, n_cells, n_keys, out.key_cell_begin);
    e = hipGetLastError();
    if (e != hipSuccess || !out.line_cell || n == 0) return e;
    hipLaunchKernelGGL(k_series_line, dim3(series_blocks(n)), dim3(256), 0, stream, n, w.cslot_of, w.rank_of_cslot, w.n_slots, out.line_cell);
    return hipGetLastError();
}

}  // namespace gx
