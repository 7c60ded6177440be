// gx_bucket.hip -- the passes of gx_bucket_lines / gx_text_bucket_lines: the lines of a finished batch counted and measured per interval
// of a number they captured, on the device.  The reference's caller does this right behind the extraction (README.md:26,63-79, with a
// timestamp field):
//     long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
//     perMinute.merge(b, 1L, Long::sum); latency.computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(...));
// The rule -- bucket_of, the word, find-or-insert, the digit plan -- is gx_bucket.hpp's; "a line counts" is gx_capture_stats'
// (gx_where_dev.hpp); the per-slot words and the workgroup's LDS table are gx_group_lines' (gx_group.hpp, gx_group_dev.hpp).
//
// 1. k_bucket_build: one lane per line, grid-stride, k_group_build's grid.  outcome -> part -> terms -> parse -> bucket -> word.  Logs are
//    time-ordered, so the lines of a wave -- of a workgroup -- share one or two buckets: the wave FIRST finds its distinct words by ballot
//    (one round per distinct word: one or two rounds), every word's lowest lane gathers what its lines add (a butterfly only where a
//    word has several lines that carry numbers) and ONLY that lane goes to the table in global memory (a 64-bit compare-and-swap where
//    the slot is still empty, else a load).  Its lines take the slot from it.  What it gathered goes to the workgroup's LDS table
//    (GROUP_LDS_ENTRIES entries, GROUP_LDS_KEYS claimable, keyed by slot), flushed once at the end of the workgroup's loop: a
//    (workgroup, bucket) costs global memory ONE group_add.  A workgroup that meets more buckets than its LDS table claims adds the
//    surplus to global memory directly.  All merges are unsigned adds and maxima of 64-bit integers: every delivered bit is the same on
//    every run.
// 2. k_bucket_flags + a scan (gx_scan.hpp): the occupied slots before every slot; [n_slots] = the buckets, read by the host in the one
//    wait in which it reads the totals.  Behind that wait k_bucket_compact writes the occupied slots' (word, slot) pairs densely.
// 3. sort: per digit of the plan: count (a workgroup owns BKT_BLOCK consecutive pairs and leaves its 64 counts, bin-major), a scan of the
//    counts, scatter (every pair to the base of its bin + its rank among the pairs before it).  The ranks come from ballots
//    (gx_radix_dev.hpp), never from atomics, and the words are distinct: the result does not depend on the waves' timing.
// 4. k_bucket_emit: one lane per rank j: bucket_number[j], bucket_first_line[j], bucket_lines[j], bucket_stats[j], rank_of_slot[slot] = j.
// 5. k_bucket_line: line_bucket[i] = rank_of_slot[slot_of[i]], 0xFFFFFFFF for a line that has no bucket.
// No workgroup waits for another, every loop is bounded by an argument or a constant.  DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_bucket.hpp"
#include "gx_bucket_sort_dev.hpp"   // the occupied flags, the compaction and the sort's kernels, shared with gx_series.hip
#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_group_dev.hpp"
#include "gx_outcome.hpp"
#include "gx_radix_dev.hpp"
#include "gx_scan.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t bucket_smem[];

// (u64, BKT_BLOCK and sort_blocks: gx_bucket_sort_dev.hpp's)

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// the table in global memory: the policy of bucket_find_or_insert on the device
struct BucketDevTable {
    u64* words;
    __device__ __forceinline__ uint64_t load(uint32_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t claim(uint32_t slot, uint64_t word) { return atomicCAS(words + slot, 0ull, static_cast<u64>(word)); }
};

// (what one slot receives: GroupAdd and group_add of gx_group_dev.hpp, as k_group_build sends them)

// LDS: BucketHead, the term image (wimage_bytes, 0: no terms), then keys[GROUP_LDS_ENTRIES], 4 words (used, spare), 8 totals (BucketDev's
// fields), and GROUP_LDS_ENTRIES x (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) 64-bit words.
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(BUCKET_WG_LINES) k_bucket_build(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                      uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ bimage,
                                                      const uint4* __restrict__ wimage, uint32_t wimage_bytes, u64* __restrict__ table, uint32_t n_slots,
                                                      u64* __restrict__ gw, u64* __restrict__ gs, uint32_t* __restrict__ slot_of, u64* __restrict__ totals) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(bucket_smem);
    uint4* b_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (sizeof(BucketHead) >> 4); q += BUCKET_WG_LINES) b_l[q] = bimage[q];
    uint4* w_l = reinterpret_cast<uint4*>(smem + sizeof(BucketHead));
    for (uint32_t q = threadIdx.x; q < (wimage_bytes >> 4); q += BUCKET_WG_LINES) w_l[q] = wimage[q];
    uint32_t* l_keys = reinterpret_cast<uint32_t*>(smem + sizeof(BucketHead) + wimage_bytes);
    uint32_t* l_used = l_keys + GROUP_LDS_ENTRIES;
    u64* l_totals = reinterpret_cast<u64*>(l_used + 4);
    u64* l_words = l_totals + 8;
    constexpr uint32_t EW = GROUP_HEAD_WORDS + GROUP_STATS_WORDS;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES; q += BUCKET_WG_LINES) l_keys[q] = GROUP_NONE;
    for (uint32_t q = threadIdx.x; q < GROUP_LDS_ENTRIES * EW; q += BUCKET_WG_LINES) l_words[q] = 0ull;
    if (threadIdx.x < 4u) l_used[threadIdx.x] = 0u;
    if (threadIdx.x < 8u) l_totals[threadIdx.x] = 0ull;
    __syncthreads();
    const BucketHead* bh = reinterpret_cast<const BucketHead*>(smem);
    const WhereHead* wh = reinterpret_cast<const WhereHead*>(smem + sizeof(BucketHead));
    const UNIT* lits = reinterpret_cast<const UNIT*>(smem + sizeof(BucketHead) + sizeof(WhereHead));
    const uint32_t n_ext = bh->n_parts;
    const bool weak = (bh->flags & GROUP_WEAK_HASH) != 0u, values = bh->has_values != 0u;
    const int64_t origin = bh->origin;
    const uint64_t width = bh->width ? bh->width : 1u;   // (it is >= 1: the host refuses the rest)
    const uint32_t ext_lo = n_ext ? bh->ext[0] : 1u, ext_hi = n_ext ? bh->ext[n_ext - 1u] : 0u;
    const bool terms = wimage_bytes != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    BucketDevTable tab{table};
    uint64_t t_lines = 0, t_unset = 0, t_nan = 0, t_oor = 0;   // (the same in every lane of the wave)
    uint32_t t_status = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * BUCKET_WG_LINES;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * BUCKET_WG_LINES + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
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
                e = where_find(bh->ext, n_ext, oc);
                if (e < n_ext && terms && !where_line_holds<F, UNIT, NUM>(wh, lits, oc, ids, caps, i, row_units, slots, data + o0, line_units)) e = n_ext;
            }
        }
        uint64_t word = 0;   // the line's bucket word; 0: it has no bucket
        uint32_t why = 0u;   // of a line that counts and has no bucket -- 1: unset, 2: no number, 3: out of range
        uint32_t cls = 3u;   // the value -- 0: a number, 1: unset, 2: no number, 3: the line has no value to measure
        int64_t v = 0;
        if (e < n_ext) {
            const GroupPart part = bh->part[e];
            int32_t pb, pe;
            pair_of<F>(ids, caps, i, row_units, slots, part.key_group, pb, pe);
            int64_t num = 0, b = 0;
            if (!where_pair_set(pb, pe, line_units)) why = 1u;
            else if (!number_parse_packed<NUM>(NUM ? bh->nfmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &num)) why = 2u;
            else if (!bucket_of(num, origin, width, &b)) why = 3u;
            else {
                word = bucket_word(b);
                if (part.value_group != GROUP_NO_VALUE) {
                    pair_of<F>(ids, caps, i, row_units, slots, part.value_group, pb, pe);
                    if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                    else cls = number_parse_packed<NUM>(NUM ? bh->vfmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                }
            }
        }
        t_lines += static_cast<uint64_t>(__popcll(__ballot(e < n_ext)));
        t_unset += static_cast<uint64_t>(__popcll(__ballot(why == 1u)));
        t_nan += static_cast<uint64_t>(__popcll(__ballot(why == 2u)));
        t_oor += static_cast<uint64_t>(__popcll(__ballot(why == 3u)));
        // the distinct words among the wave's 64 lines: every word's lowest lane gathers what its lines add, and leads them to the table
        GroupAdd add{};
        bool leader = false;
        uint32_t lead = lane;
        uint64_t todo = __ballot(word != 0ull);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<u64>(todo))) - 1u;
            const uint64_t ww = static_cast<uint64_t>(__shfl(static_cast<u64>(word), static_cast<int>(l)));
            const bool mine = word == ww;   // (ww != 0: a lane without a bucket is nobody's)
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
                if (numbers && (members & (members - 1ull))) {            // (several lines in the bucket: a butterfly; one line has its own)
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        lo += wave_xor64(lo, d);
                        hi += wave_xor64(hi, d);
                        mn = umax64(mn, wave_xor64(mn, d));
                        mx = umax64(mx, wave_xor64(mx, d));
                    }
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
        uint32_t slot = GROUP_NONE;
        if (leader) {
            slot = bucket_find_or_insert(tab, n_slots, word, weak);
            if (slot == GROUP_NONE) t_status |= 2u;
        }
        slot = static_cast<uint32_t>(__shfl(static_cast<int>(slot), static_cast<int>(lead)));   // (a lane without a bucket leads itself: GROUP_NONE)
        if (valid) slot_of[i] = slot;
        if (leader && slot != GROUP_NONE) {
            atomicMax(l_totals + 5, static_cast<u64>(~word));
            atomicMax(l_totals + 6, static_cast<u64>(word));
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
        if (t_nan) atomicAdd(l_totals + 3, static_cast<u64>(t_nan));
        if (t_oor) atomicAdd(l_totals + 4, static_cast<u64>(t_oor));
    }
    // (status: every lane has its own bits)
    const uint64_t any1 = __ballot((t_status & 1u) != 0u), any2 = __ballot((t_status & 2u) != 0u);
    if (lane == 0u && (any1 | any2)) atomicOr(l_totals + 2, static_cast<u64>((any1 ? 1u : 0u) | (any2 ? 2u : 0u)));
    __syncthreads();
    if (threadIdx.x < 7u && l_totals[threadIdx.x]) {
        if (threadIdx.x == 2u) atomicOr(totals + 2, l_totals[2]);
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
        group_add(gw + static_cast<uint64_t>(s) * GROUP_HEAD_WORDS, gs + static_cast<uint64_t>(s) * GROUP_STATS_WORDS, values, a);
    }
}

// One lane per rank j: the bucket's row and its slot's rank.  m <= the per-bucket arrays' capacity (the host has checked it).
__global__ void __launch_bounds__(256) k_bucket_emit(const uint64_t* __restrict__ word, const uint32_t* __restrict__ slot, uint32_t m, uint32_t n_slots,
                                                     const u64* __restrict__ gw, const u64* __restrict__ gs, uint32_t* __restrict__ rank_of_slot, BucketOut out) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t s = slot[j];
    if (s >= n_slots) return;   // (it is not: the compaction wrote slot numbers)
    rank_of_slot[s] = static_cast<uint32_t>(j);
    if (out.bucket_number) out.bucket_number[j] = bucket_number(word[j]);
    if (out.bucket_first_line) out.bucket_first_line[j] = group_first_line(gw[static_cast<uint64_t>(s) * GROUP_HEAD_WORDS + GROUP_W_FIRST]);
    if (out.bucket_lines) out.bucket_lines[j] = gw[static_cast<uint64_t>(s) * GROUP_HEAD_WORDS + GROUP_W_LINES];
    if (out.bucket_stats) {
        uint64_t w[GROUP_STATS_WORDS], st[8];
#pragma unroll
        for (uint32_t q = 0; q < GROUP_STATS_WORDS; ++q) w[q] = gs[static_cast<uint64_t>(s) * GROUP_STATS_WORDS + q];
        group_stats_out(w, st);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) out.bucket_stats[j * 8u + q] = st[q];
    }
}

__global__ void __launch_bounds__(256) k_bucket_line(uint64_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ rank_of_slot, uint32_t n_slots,
                                                     uint32_t* __restrict__ line_bucket) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_of[i];
        line_bucket[i] = slot < n_slots ? rank_of_slot[slot] : GROUP_NONE;
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_build_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const GroupArgs& a, const BucketWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *bi = static_cast<const uint4*>(a.image), *wi = static_cast<const uint4*>(a.where_image);
    u64 *table = reinterpret_cast<u64*>(w.table), *gw = reinterpret_cast<u64*>(w.head_words), *gs = reinterpret_cast<u64*>(w.stats_words),
        *totals = reinterpret_cast<u64*>(w.totals);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_bucket_build<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, bi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_bucket_build<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, bi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, totals);
    else
        hipLaunchKernelGGL((k_bucket_build<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(BUCKET_WG_LINES), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, bi, wi,
                           a.where_image_bytes, table, w.n_slots, gw, gs, w.slot_of, totals);
}

unsigned bucket_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048)); }
static_assert(BUCKET_WG_LINES == 256, "bucket_blocks gives the build pass one workgroup per 256 lines");
uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }

}  // namespace

// The slots' words -- zeroed before every call by ONE memset: [table n_slots][head 2 n_slots][stats 8 n_slots, with values][totals 8],
// all 64-bit -- then before[n_slots + 1], the scan's sums, rank_of_slot[n_slots] and occupied[n_slots]: 29 bytes per slot, 93 with values.
size_t bucket_table_zero_bytes(uint32_t n_slots, bool values) {
    return (static_cast<size_t>(n_slots) * (1u + GROUP_HEAD_WORDS + (values ? GROUP_STATS_WORDS : 0u)) + 8u) * 8u;
}
size_t bucket_table_bytes(uint32_t n_slots, bool values) {
    return bucket_table_zero_bytes(n_slots, values) + pad16((static_cast<uint64_t>(n_slots) + 1u) * 8u) + scan_sums_bytes(n_slots) +
           pad16(static_cast<uint64_t>(n_slots) * 4u) + pad16(n_slots);
}
// the per-line array: slot_of (32-bit)
size_t bucket_lines_bytes(uint64_t n) { return pad16(n * 4u); }

BucketWs bucket_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, bool values) {
    (void)n;
    BucketWs w{};
    w.n_slots = n_slots;
    uint64_t* t = static_cast<uint64_t*>(table_mem);
    w.table = t;
    w.head_words = t + n_slots;
    w.stats_words = w.head_words + static_cast<size_t>(n_slots) * GROUP_HEAD_WORDS;   // (never touched without values)
    w.totals = w.stats_words + (values ? static_cast<size_t>(n_slots) * GROUP_STATS_WORDS : 0u);
    uint8_t* p = reinterpret_cast<uint8_t*>(w.totals + 8);
    w.before = reinterpret_cast<uint64_t*>(p); p += pad16((static_cast<uint64_t>(n_slots) + 1u) * 8u);
    w.sums = reinterpret_cast<uint64_t*>(p); p += scan_sums_bytes(n_slots);
    w.rank_of_slot = reinterpret_cast<uint32_t*>(p); p += pad16(static_cast<uint64_t>(n_slots) * 4u);
    w.occupied = p;
    w.slot_of = static_cast<uint32_t*>(lines_mem);
    return w;
}

// The sort's workspace for m buckets: the words and the slots, ping and pong (24 bytes per bucket), and 768 bytes per BKT_BLOCK
// buckets of counts and bases.
BucketSortWs bucket_sort_workspace(void* ws, uint64_t m) {
    const uint64_t slab = 64u * sort_blocks(m);
    BucketSortWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    for (int q = 0; q < 2; ++q) w.word[q] = reinterpret_cast<uint64_t*>(take(m * 8u));
    for (int q = 0; q < 2; ++q) w.slot[q] = reinterpret_cast<uint32_t*>(take(m * 4u));
    w.bases = reinterpret_cast<uint64_t*>(take((slab + 1u) * 8u));
    w.block_sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(slab)));
    w.slab = reinterpret_cast<uint32_t*>(take(slab * 4u));
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t bucket_sort_workspace_bytes(uint64_t m) { return bucket_sort_workspace(nullptr, m).bytes; }

// Passes 1 and 2 on `stream`, n > 0 and parts > 0: leaves w.totals (BucketDev) and w.before[n_slots] = the buckets.  The part image (and
// the term image, if any) are on the device.
hipError_t launch_bucket_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const BucketWs& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.table, 0, bucket_table_zero_bytes(w.n_slots, a.has_values != 0), stream);
    if (e != hipSuccess) return e;
    const uint32_t lds = static_cast<uint32_t>(sizeof(BucketHead)) + a.where_image_bytes + GROUP_LDS_ENTRIES * 4u + 16u + 64u +
                         GROUP_LDS_ENTRIES * (GROUP_HEAD_WORDS + GROUP_STATS_WORDS) * 8u;
    if (lds > 64u * 1024u) return hipErrorInvalidValue;   // (64 terms of 255 two-byte units: 34 KiB; BucketHead and the LDS table: 11.4 KiB)
    const unsigned blocks = bucket_blocks(n);
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
    hipLaunchKernelGGL(k_bucket_flags, dim3(bucket_blocks(w.n_slots)), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.table), w.n_slots, w.occupied);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint8_t>(w.occupied, w.n_slots, w.sums, w.before, stream);
}

// Passes 2 (the pairs), 3, 4 and 5 on `stream`, behind launch_bucket_build and the host's read of m = w.before[n_slots] (0 < m <= n_slots,
// m <= the per-bucket arrays' capacity) and of the smallest and largest word (n_digits: bucket_digits of them, or all of them).
hipError_t launch_bucket_emit(uint64_t n, uint64_t m, uint32_t n_digits, const BucketWs& w, const BucketSortWs& s, const BucketOut& out, hipStream_t stream) {
    if (m == 0 || m > w.n_slots || n_digits > BUCKET_MAX_DIGITS) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    const uint64_t blocks64 = sort_blocks(m);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    hipLaunchKernelGGL(k_bucket_compact, dim3(bucket_blocks(w.n_slots)), dim3(256), 0, stream, reinterpret_cast<const u64*>(w.table), w.n_slots, w.occupied, w.before,
                       m32, s.word[0], s.slot[0]);
    uint32_t cur = 0;
    for (uint32_t d = 0; d < n_digits; ++d) {
        hipLaunchKernelGGL(k_bucket_count, dim3(blocks), dim3(256), 0, stream, s.word[cur], m32, d, s.slab);
        const hipError_t e = launch_exclusive_scan<uint32_t>(s.slab, 64u * blocks64, s.block_sums, s.bases, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bucket_scatter, dim3(blocks), dim3(256), 0, stream, s.word[cur], s.slot[cur], m32, d, s.bases, s.word[cur ^ 1u], s.slot[cur ^ 1u]);
        cur ^= 1u;
    }
    hipLaunchKernelGGL(k_bucket_emit, dim3(static_cast<unsigned>((m + 255) / 256)), dim3(256), 0, stream, s.word[cur], s.slot[cur], m32, w.n_slots,
                       reinterpret_cast<const u64*>(w.head_words), reinterpret_cast<const u64*>(w.stats_words), w.rank_of_slot, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out.line_bucket || n == 0) return e;
    hipLaunchKernelGGL(k_bucket_line, dim3(bucket_blocks(n)), dim3(256), 0, stream, n, w.slot_of, w.rank_of_slot, w.n_slots, out.line_bucket);
    return hipGetLastError();
}

}  // namespace gx
