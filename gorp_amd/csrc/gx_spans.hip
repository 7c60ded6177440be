// gx_spans.hip -- the passes of gx_group_spans / gx_text_group_spans: a key's BEGIN and END lines paired in input order, on the device.
// The reference's caller does this behind the extraction with a map of open requests: put on a start line, remove on an end line.
// The rule -- which lines are entries, the states, the exact duration -- is gx_spans.hpp; the pair sort's kernels are
// gx_bucket_sort_dev.hpp's, the scan is gx_scan.hpp's.  All passes run behind launch_group_build (gx_group.hip), which leaves slot_of[],
// the slots' first lines and idx_off[] complete and is not changed: a key's NUMBER is idx_off[its first line], which is what
// launch_group_emit later writes to keynum[] -- so nothing here waits for the emit, and the host can refuse a capacity before ANY output
// is written.
//
// Before the host's first wait, the one in which it reads gx_group_lines' totals (launch_spans_entries):
//   entries  one lane per line, grid-stride.  Lines without a key slot are skipped; the others count and are keyed, so no term is
//            evaluated again.  outcome -> part -> role, number pair -> parse: the entry flag, the time's class and the role in one
//            byte, the time.
//   scan     before[i] = the entries before line i; before[n] = the entries (the keyed lines).
// Behind that wait, sized by the entries m and the keys read there (launch_spans_pair):
//   compact  (key number, line) pairs, dense, in line order.
//   sort     ONE stable sort by the key number's digits: (key, line) order.
//   heads    one lane per entry e, a wave over 64 consecutive entries: the entries e - 1 and e + 1 come from the neighbouring lanes, and
//            for a wave's first and last lane from global memory -- so the read crosses wave, workgroup, sort-block and scan-tile edges
//            alike.  state[e] (span_state), flag[e] = e ends a span; for a span its exact duration as four columns for four scans -- a
//            key's and the batch's sums are differences of prefix sums, exact modulo 2^64 as gx_group.hip's adds are -- and its minimum
//            and maximum reduced inside the wave over runs of equal key (six shuffle steps), merged per run and wave by an integer
//            atomic maximum.  The states' counts: ballots per wave, LDS per workgroup, one integer atomic per word and workgroup.
//   scans    sbefore[e] = the spans that end before entry e; sbefore[m] = the spans.  pre[q][e] likewise of the four columns.
// The host reads n_spans, the counts and the batch's sums in the call's SECOND wait and checks the capacities.  Then (launch_spans_emit):
//   emit     one lane per entry: a span's end writes the span's row (the begin is the entry before it), every entry its line's state
//            and span behind fills with "none".
//   keys     one lane per key j: its entries' run by lower bound over the sorted key numbers; key_span_begin[j] = sbefore[run's first],
//            key_open_line[j] from the run's last entry, key_span_stats[j] from the prefix sums' differences and the merged maxima.
// No workgroup waits for another, every loop is bounded by an argument or a constant, every value is written by an ordinary vector
// store or an integer atomic.  DESIGN.md section 5.4.
//
// The workspace: per input line 8 (time) + 8 (scan) + 1 (flag) + 1 (class and role) = 18 bytes; per entry 2 x 12 (the sort's ping and
// pong) + 1 (state) + 1 (flag) + 8 (scan) + 4 x 16 (four columns and their scans) = 98 bytes and 768 per 2 048 entries of counts and
// bases; per key 16 (minimum and maximum); per span nothing.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <hip/hip_runtime.h>

#include "gx_bucket_sort_dev.hpp"
#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_outcome.hpp"
#include "gx_scan.hpp"
#include "gx_spans.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

// (of gx_bucket_sort_dev.hpp this file launches the pair sort's two kernels; the table's two are gx_bucket.hip's and gx_series.hip's)
[[maybe_unused]] const auto not_launched_here = std::make_pair(&k_bucket_flags, &k_bucket_compact);

constexpr uint32_t SPAN_LINE_BLOCKS = 2048;

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_span_entries(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                      uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                      const uint4* __restrict__ simage, const uint32_t* __restrict__ slot_of, int64_t* __restrict__ tval,
                                                      uint8_t* __restrict__ ent, uint8_t* __restrict__ tcr) {
    __shared__ uint4 g_l[sizeof(GroupHead) >> 4];
    __shared__ uint4 s_l[sizeof(SpansHead) >> 4];
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    for (uint32_t q = threadIdx.x; q < (sizeof(SpansHead) >> 4); q += 256u) s_l[q] = simage[q];
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(g_l);
    const SpansHead* sh = reinterpret_cast<const SpansHead*>(s_l);
    const uint32_t n_ext = gh->n_parts;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const bool keyed = slot_of[i] != GROUP_NONE;   // (the line counts and its key pair is set: the build found it so)
        ent[i] = keyed ? 1 : 0;
        if (!keyed) continue;
        const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
        const uint32_t e = where_find(gh->ext, n_ext, oc);
        const bool part = e < n_ext;   // (it is: a keyed line's outcome has a part)
        const int32_t ng = part ? sh->number[e] : SPANS_NO_NUMBER;
        const uint32_t role = part ? sh->role[e] : SPAN_END;
        uint32_t cls = SPAN_C_UNSET;
        int64_t num = 0;
        if (ng >= 0) {
            const uint64_t o0 = static_cast<uint64_t>(off[i]);
            const uint64_t line_units = static_cast<uint64_t>(off[i + 1]) - o0;   // (< 4 G: the build gives no key to a longer line)
            int32_t pb, pe;
            pair_of<F>(ids, caps, i, row_units, slots, static_cast<uint32_t>(ng), pb, pe);
            if (where_pair_set(pb, pe, line_units))
                cls = number_parse_packed<NUM>(NUM ? sh->nfmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &num) ? SPAN_C_NUMBER
                                                                                                                                                    : SPAN_C_NAN;
        }
        tcr[i] = span_pack(cls, role);
        tval[i] = cls == SPAN_C_NUMBER ? num : 0;
    }
}

// kword[at], line[at] = line i's key number and i, at = the entries before line i; m: the entries the host read from the same scan.  A
// key's number is idx_off[its first line]: what launch_group_emit writes to keynum[] of the slot.
__global__ void __launch_bounds__(256) k_span_compact(uint64_t n, const uint8_t* __restrict__ ent, const uint64_t* __restrict__ before,
                                                      const uint32_t* __restrict__ slot_of, uint32_t n_slots, const u64* __restrict__ gw,
                                                      const uint64_t* __restrict__ idx_off, uint32_t m, uint64_t* __restrict__ kword, uint32_t* __restrict__ line) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!ent[i]) continue;
        const uint64_t at = before[i];
        if (at >= m) continue;   // (it is not: the scan counted these very flags, and the host read m from it)
        uint64_t j = 0;
        const uint32_t slot = slot_of[i];
        if (slot < n_slots) {   // (it is: an entry has a key)
            const uint32_t first = group_first_line(gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_FIRST]);
            if (first < n) j = idx_off[first];
        }
        kword[at] = j;
        line[at] = static_cast<uint32_t>(i);
    }
}

// One lane per entry e of the (key, line) order, a wave over 64 consecutive entries: kword[e] its key number, line[e] its line, whose
// class, role and time the entries pass left in tcr[] and tval[].  (kmin / kmax: n_keys words each, zeroed; dev zeroed.)
__global__ void __launch_bounds__(256) k_span_heads(const uint64_t* __restrict__ kword, const uint32_t* __restrict__ line, uint32_t m, uint64_t n,
                                                    const uint8_t* __restrict__ tcr, const int64_t* __restrict__ tval, uint64_t n_keys, uint8_t* __restrict__ state,
                                                    uint8_t* __restrict__ flag, uint64_t* __restrict__ c_counts, uint64_t* __restrict__ c_nan,
                                                    uint64_t* __restrict__ c_lo, uint64_t* __restrict__ c_hi, u64* __restrict__ kmin, u64* __restrict__ kmax,
                                                    u64* __restrict__ dev) {
    __shared__ u64 l_dev[sizeof(SpansDev) / 8];
    if (threadIdx.x < sizeof(SpansDev) / 8) l_dev[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t_state[SPAN_STATES] = {0, 0, 0, 0, 0, 0};   // (the same in every lane of the wave)
    uint64_t w_min = 0, w_max = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e0 = blockIdx.x * 256u + (threadIdx.x & ~63u); e0 < m; e0 += stride) {
        const uint32_t e = e0 + lane;
        const bool valid = e < m;
        uint32_t key = GROUP_NONE, role = 0u, cls = SPAN_C_UNSET;
        int64_t t = 0;
        if (valid) {
            key = static_cast<uint32_t>(kword[e]);
            const uint32_t i = line[e];
            if (i < n) {   // (it is: a line number of the batch)
                const uint8_t b = tcr[i];
                role = span_pack_role(b);
                cls = span_pack_class(b);
                t = tval[i];
            }
        }
        // the entry before and the entry behind: the neighbouring lanes', and at the wave's two ends global memory's
        const bool has_prev = valid && e > 0u, has_next = valid && e + 1u < m;
        uint32_t pkey = static_cast<uint32_t>(__shfl_up(static_cast<int>(key), 1)), prole = static_cast<uint32_t>(__shfl_up(static_cast<int>(role), 1));
        uint32_t pcls = static_cast<uint32_t>(__shfl_up(static_cast<int>(cls), 1));
        int64_t pt = static_cast<int64_t>(__shfl_up(static_cast<long long>(t), 1));
        uint32_t nkey = static_cast<uint32_t>(__shfl_down(static_cast<int>(key), 1)), nrole = static_cast<uint32_t>(__shfl_down(static_cast<int>(role), 1));
        if (lane == 0u && has_prev) {
            pkey = static_cast<uint32_t>(kword[e - 1u]);
            const uint32_t i = line[e - 1u];
            prole = 0u;
            pcls = SPAN_C_UNSET;
            pt = 0;
            if (i < n) {
                const uint8_t b = tcr[i];
                prole = span_pack_role(b);
                pcls = span_pack_class(b);
                pt = tval[i];
            }
        }
        if (lane == 63u && has_next) {
            nkey = static_cast<uint32_t>(kword[e + 1u]);
            const uint32_t i = line[e + 1u];
            nrole = i < n ? span_pack_role(tcr[i]) : 0u;
        }
        const uint32_t st = valid ? span_state(role, has_prev && pkey == key, prole, has_next && nkey == key, nrole) : SPAN_S_NONE;
        const bool is_end = st == SPAN_S_END;
        SpanRow r{0, 0, 0, SPAN_C_UNSET, false};
        if (is_end) r = span_row(pcls, pt, cls, t);
        const bool number = is_end && r.cls == SPAN_C_NUMBER;
        if (valid) {
            state[e] = static_cast<uint8_t>(st);
            flag[e] = is_end ? 1 : 0;
            c_counts[e] = (number ? 1ull : 0ull) | (is_end && r.cls == SPAN_C_UNSET ? (1ull << 32) : 0ull);
            c_nan[e] = (is_end && r.cls == SPAN_C_NAN ? 1ull : 0ull) | (r.out_of_range ? (1ull << 32) : 0ull);
            c_lo[e] = number ? (static_cast<uint64_t>(r.duration) & 0xFFFFFFFFull) : 0ull;
            c_hi[e] = number ? static_cast<uint64_t>(stats_high(r.duration)) : 0ull;   // (two's complement: adds as unsigned)
        }
#pragma unroll
        for (uint32_t q = 1; q < SPAN_STATES; ++q) t_state[q] += static_cast<uint64_t>(__popcll(__ballot(st == q)));
        // the maxima over the run of equal key that ends at this lane (the key numbers ascend along the wave); 0, "no number", is the
        // identity of the maximum, and group_stats_out looks at a word only where the key has a number
        uint64_t a = number ? group_min_word(r.duration) : 0ull, b = number ? group_max_word(r.duration) : 0ull;
        w_min = umax64(w_min, a);
        w_max = umax64(w_max, b);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ok = static_cast<uint32_t>(__shfl_up(static_cast<int>(key), d));
            const uint64_t oa = static_cast<uint64_t>(__shfl_up(static_cast<u64>(a), d)), ob = static_cast<uint64_t>(__shfl_up(static_cast<u64>(b), d));
            if (lane >= static_cast<uint32_t>(d) && ok == key) {
                a = umax64(a, oa);
                b = umax64(b, ob);
            }
        }
        const uint32_t after = static_cast<uint32_t>(__shfl_down(static_cast<int>(key), 1));
        const bool run_last = valid && (lane == 63u || after != key);
        if (run_last && key < n_keys) {   // (key < n_keys: a key number)
            if (a) atomicMax(kmin + key, static_cast<u64>(a));
            if (b) atomicMax(kmax + key, static_cast<u64>(b));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        w_min = umax64(w_min, wave_xor64(w_min, d));
        w_max = umax64(w_max, wave_xor64(w_max, d));
    }
    if (lane == 0u) {
#pragma unroll
        for (uint32_t q = 1; q < SPAN_STATES; ++q)
            if (t_state[q]) atomicAdd(l_dev + q, static_cast<u64>(t_state[q]));
        if (w_min) atomicMax(l_dev + SPAN_STATES, static_cast<u64>(w_min));
        if (w_max) atomicMax(l_dev + SPAN_STATES + 1u, static_cast<u64>(w_max));
    }
    __syncthreads();
    if (threadIdx.x < sizeof(SpansDev) / 8 && l_dev[threadIdx.x]) {
        if (threadIdx.x >= SPAN_STATES) atomicMax(dev + threadIdx.x, l_dev[threadIdx.x]);
        else atomicAdd(dev + threadIdx.x, l_dev[threadIdx.x]);
    }
}

// One lane per entry e.  A span's end (flag[e]) writes row sbefore[e] < ns (the host has checked ns against the capacity); the begin is
// entry e - 1.  Every entry writes its line's state and span (behind fills with 0 and "none").
__global__ void __launch_bounds__(256) k_span_emit(const uint64_t* __restrict__ kword, const uint32_t* __restrict__ line, uint32_t m, uint64_t n, uint32_t ns,
                                                   const uint8_t* __restrict__ tcr, const int64_t* __restrict__ tval, const uint8_t* __restrict__ state,
                                                   const uint8_t* __restrict__ flag, const uint64_t* __restrict__ sbefore, SpansOut out) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        const uint32_t i = line[e];
        const uint32_t st = state[e];
        const uint64_t s = st == SPAN_S_BEGIN ? sbefore[e + 1u] : sbefore[e];   // (a span's begin: the entry behind it ends the span)
        if (i < n) {   // (it is: a line number of the batch)
            if (out.line_state) out.line_state[i] = static_cast<uint8_t>(st);
            if (out.line_span && (st == SPAN_S_BEGIN || st == SPAN_S_END) && s < ns) out.line_span[i] = static_cast<uint32_t>(s);
        }
        if (!flag[e] || e == 0u || s >= ns || i >= n) continue;   // (a flagged entry has one before it; s < ns: the scan counted these flags)
        const uint32_t ib = line[e - 1u];
        if (ib >= n) continue;
        const uint8_t bb = tcr[ib], be = tcr[i];
        const SpanRow r = span_row(span_pack_class(bb), tval[ib], span_pack_class(be), tval[i]);
        if (out.span_key) out.span_key[s] = static_cast<uint32_t>(kword[e]);
        if (out.span_begin_line) out.span_begin_line[s] = ib;
        if (out.span_end_line) out.span_end_line[s] = i;
        if (out.span_begin) out.span_begin[s] = r.begin;
        if (out.span_end) out.span_end[s] = r.end;
        if (out.span_duration) out.span_duration[s] = r.duration;
        if (out.span_class) out.span_class[s] = static_cast<uint8_t>(r.cls);
    }
}

// One lane per key j in 0 .. n_keys: its entries are [by_key_begin(j), by_key_begin(j + 1)) of the sorted order; [n_keys] = the spans.
__global__ void __launch_bounds__(256) k_span_keys(const uint64_t* __restrict__ kword, const uint32_t* __restrict__ line, uint32_t m, uint64_t n_keys,
                                                   const uint8_t* __restrict__ state, const uint64_t* __restrict__ sbefore, const uint64_t* __restrict__ p_counts,
                                                   const uint64_t* __restrict__ p_nan, const uint64_t* __restrict__ p_lo, const uint64_t* __restrict__ p_hi,
                                                   const u64* __restrict__ kmin, const u64* __restrict__ kmax, SpansOut out) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > n_keys) return;
    const uint64_t b = by_key_begin(kword, m, j);
    if (out.key_span_begin) out.key_span_begin[j] = sbefore[b];
    if (j == n_keys) return;
    const uint64_t e = by_key_begin(kword, m, j + 1u);
    if (out.key_open_line) out.key_open_line[j] = e > b && state[e - 1u] == SPAN_S_OPEN ? line[e - 1u] : GROUP_NONE;
    if (out.key_span_stats) {
        const uint64_t c = p_counts[e] - p_counts[b], x = p_nan[e] - p_nan[b];
        uint64_t w[GROUP_STATS_WORDS], st[8];
        w[GROUP_S_NUMBERS] = c & 0xFFFFFFFFull;
        w[GROUP_S_UNSET] = c >> 32;
        w[GROUP_S_NOT_NUMBERS] = x & 0xFFFFFFFFull;
        w[GROUP_S_MIN] = kmin[j];
        w[GROUP_S_MAX] = kmax[j];
        w[GROUP_S_LO] = p_lo[e] - p_lo[b];
        w[GROUP_S_HI] = p_hi[e] - p_hi[b];
        w[GROUP_S_SPARE] = 0ull;
        group_stats_out(w, st);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) out.key_span_stats[j * 8u + q] = st[q];
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_entries_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off, const GroupArgs& a,
                       const GroupWs& g, const SpansWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *si = reinterpret_cast<const uint4*>(w.image);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_span_entries<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tval, w.ent, w.tcr);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_span_entries<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tval, w.ent, w.tcr);
    else
        hipLaunchKernelGGL((k_span_entries<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tval, w.ent, w.tcr);
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
unsigned line_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, SPAN_LINE_BLOCKS)); }

}  // namespace

SpansWs spans_workspace(void* ws, uint64_t n) {
    SpansWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.image = take(sizeof(SpansHead));
    w.tval = reinterpret_cast<int64_t*>(take(n * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(n)));
    w.ent = take(n);
    w.tcr = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t spans_workspace_bytes(uint64_t n) { return spans_workspace(nullptr, n).bytes; }

SpansPairWs spans_pair_workspace(void* ws, uint64_t m, uint64_t n_keys) {
    SpansPairWs s{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    s.dev = take(sizeof(SpansDev));
    s.sort = bucket_sort_workspace(take(bucket_sort_workspace_bytes(m)), m);
    s.sbefore = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
    s.sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(m)));
    for (int q = 0; q < 4; ++q) s.col[q] = reinterpret_cast<uint64_t*>(take(m * 8));
    for (int q = 0; q < 4; ++q) s.pre[q] = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
    s.kmin = reinterpret_cast<uint64_t*>(take(n_keys * 16));
    s.kmax = s.kmin + n_keys;
    s.state = take(m);
    s.flag = take(m);
    s.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return s;
}
size_t spans_pair_workspace_bytes(uint64_t m, uint64_t n_keys) { return spans_pair_workspace(nullptr, m, n_keys).bytes; }

// The entries pass and the scan on `stream`, n > 0 and parts > 0, behind launch_group_build: leaves w.before[n] = the entries.  a.image
// (GroupHead) and w.image (SpansHead) are on the device.
hipError_t launch_spans_entries(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                bool formats, const GroupWs& g, const SpansWs& w, hipStream_t stream) {
    const unsigned blocks = line_blocks(n);
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (formats) launch_entries_as<OFF, UNIT, true>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w);
        else launch_entries_as<OFF, UNIT, false>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, g, w);
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
    return launch_exclusive_scan<uint8_t>(w.ent, n, w.sums, w.before, stream);
}

// Behind launch_spans_entries and the host's read of the entries and of n_keys on `stream`: 0 < m <= min(n, 2^30) entries, 0 < n_keys
// keys, the key sort's digits.  Leaves the (key, line) order in s.sort.word[*buf] / .slot[*buf], state[], flag[], sbefore[], the four
// columns' scans and SpansDev at s.dev.
hipError_t launch_spans_pair(uint64_t n, uint64_t m, uint64_t n_keys, uint32_t key_digits, const GroupWs& g, const SpansWs& w, const SpansPairWs& s, uint32_t* buf,
                             hipStream_t stream) {
    if (m == 0 || m > n || m > SPANS_MAX || n_keys == 0 || n_keys > m || key_digits > BY_KEY_MAX_PASSES) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    hipError_t e = hipMemsetAsync(s.dev, 0, sizeof(SpansDev), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s.kmin, 0, n_keys * 16, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_span_compact, dim3(line_blocks(n)), dim3(256), 0, stream, n, w.ent, w.before, g.slot_of, g.n_slots, reinterpret_cast<const u64*>(g.head_words),
                       g.idx_off, m32, s.sort.word[0], s.sort.slot[0]);
    const uint64_t blocks64 = sort_blocks(m32);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    uint32_t cur = 0;
    for (uint32_t d = 0; d < key_digits; ++d) {
        hipLaunchKernelGGL(k_bucket_count, dim3(blocks), dim3(256), 0, stream, s.sort.word[cur], m32, d, s.sort.slab);
        e = launch_exclusive_scan<uint32_t>(s.sort.slab, 64u * blocks64, s.sort.block_sums, s.sort.bases, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bucket_scatter, dim3(blocks), dim3(256), 0, stream, s.sort.word[cur], s.sort.slot[cur], m32, d, s.sort.bases, s.sort.word[cur ^ 1u],
                           s.sort.slot[cur ^ 1u]);
        cur ^= 1u;
    }
    hipLaunchKernelGGL(k_span_heads, dim3(line_blocks(m)), dim3(256), 0, stream, s.sort.word[cur], s.sort.slot[cur], m32, n, w.tcr, w.tval, n_keys, s.state, s.flag,
                       s.col[0], s.col[1], s.col[2], s.col[3], reinterpret_cast<u64*>(s.kmin), reinterpret_cast<u64*>(s.kmax), reinterpret_cast<u64*>(s.dev));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(s.flag, m, s.sums, s.sbefore, stream);
    if (e != hipSuccess) return e;
    for (int q = 0; q < 4; ++q) {
        e = launch_exclusive_scan<uint64_t>(s.col[q], m, s.sums, s.pre[q], stream);
        if (e != hipSuccess) return e;
    }
    *buf = cur;
    return hipGetLastError();
}

// Behind launch_spans_pair and the host's read of the spans and check of the capacities: ns spans (ns <= m / 2), n_keys keys.  buf: what
// launch_spans_pair left.
hipError_t launch_spans_emit(uint64_t n, uint64_t m, uint64_t ns, uint64_t n_keys, const SpansWs& w, const SpansPairWs& s, uint32_t buf, const SpansOut& out,
                             hipStream_t stream) {
    if (m == 0 || m > SPANS_MAX || ns > m || buf > 1u) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    const uint64_t* kword = s.sort.word[buf];
    const uint32_t* line = s.sort.slot[buf];
    hipError_t e = hipSuccess;
    if (out.line_span && (e = hipMemsetAsync(out.line_span, 0xFF, n * 4, stream)) != hipSuccess) return e;
    if (out.line_state && (e = hipMemsetAsync(out.line_state, 0, n, stream)) != hipSuccess) return e;
    const bool per_span = out.span_key || out.span_begin_line || out.span_end_line || out.span_begin || out.span_end || out.span_duration || out.span_class;
    if (per_span || out.line_span || out.line_state)
        hipLaunchKernelGGL(k_span_emit, dim3(line_blocks(m)), dim3(256), 0, stream, kword, line, m32, n, static_cast<uint32_t>(ns), w.tcr, w.tval, s.state, s.flag,
                           s.sbefore, out);
    if (out.key_span_begin || out.key_span_stats || out.key_open_line)
        hipLaunchKernelGGL(k_span_keys, dim3(static_cast<unsigned>((n_keys + 1 + 255) / 256)), dim3(256), 0, stream, kword, line, m32, n_keys, s.state, s.sbefore,
                           s.pre[0], s.pre[1], s.pre[2], s.pre[3], reinterpret_cast<const u64*>(s.kmin), reinterpret_cast<const u64*>(s.kmax), out);
    return hipGetLastError();
}

}  // namespace gx
