// gx_sessions.hip -- the passes of gx_group_sessions / gx_text_group_sessions: a key's lines ordered by a captured time and cut into
// sessions wherever the time steps by more than max_gap, on the device.  The reference's caller does this behind the extraction
// (README.md:26,63-79): byId.computeIfAbsent(id, ...).add(r); per id sort by ts; a new session wherever ts - previous ts > maxGap.
// The rule -- which lines are entries, the gap test, the digit plans -- is gx_sessions.hpp; the pair sort's kernels are
// gx_bucket_sort_dev.hpp's, the scan is gx_scan.hpp's.  All passes run behind launch_group_build (gx_group.hip), which leaves slot_of[],
// the slots' first lines and idx_off[] complete and is not changed: a key's NUMBER is idx_off[its first line], which is what
// launch_group_emit later writes to keynum[] -- so nothing here waits for the emit, and the host can refuse a capacity before ANY output
// is written.
//
// Before the host's first wait, the one in which it reads gx_group_lines' totals (launch_sessions_keys):
//   keys     one lane per line, grid-stride.  Lines without a key slot are skipped; the others count and are keyed, so no term is
//            evaluated again.  outcome -> part -> number pair -> parse: the entry flag and the time word (top_key); with a value group
//            also the value and its class.  (gx_top.hip's keys pass classes the lines that COUNT; number_unset and not_numbers are over
//            the KEYED lines, so this pass stands on slot_of[] as k_series_build does.)  The class counts and the OR / AND / minimum /
//            maximum of the time words: ballots and a butterfly per wave, LDS per workgroup, one integer atomic per word and workgroup.
//   scan     before[i] = the entries before line i.
// Behind that wait, sized by the entries m read there (launch_sessions_sort):
//   compact  (time word, line) pairs, dense, in line order.
//   sort     by the digits of the time words that differ (sessions_time_plan): (time, line) order.
//   number   (key number, place in time order) pairs; the second stable sort over the key number's digits: (key, time, line) order.
//   heads    one lane per entry e: its time and line gathered into that order, and head[e] (session_head); the entry before a
//            workgroup's first is read from global memory like any other.
//   scan     sbefore[e] = the heads before entry e; sbefore[m] = the sessions.
//   starts   start[s] = the first entry of session s; start[n_sessions] = m.
//   longest  one lane per session: its entries and its duration, the maxima by integer atomics.
// The host reads n_sessions and the maxima in the call's SECOND wait and checks the capacities.  Then (launch_sessions_emit):
//   values   (with session_stats) one lane per entry: the value's class counts and the two halves of its 128-bit sum as four columns
//            for four scans -- a session's sum is the difference of two prefix sums, exact modulo 2^64 as gx_group.hip's adds are --
//            and the minimum and maximum reduced inside the wave over runs of equal session number (six shuffle steps), merged per run
//            and wave by an integer atomic maximum: a session may hold one entry or all of them, no lane loops over a session.
//   emit     one lane per session: key, begin, end, first line, entries, stats, session_entry_begin.
//   bounds   key_session_begin[j] by lower bound over the sessions' key numbers (a key without an entry has an empty run).
//   lines    entry_line[e], and line_session[] by scatter through it behind a fill with "none".
// No workgroup waits for another, every loop is bounded by an argument or a constant, every value is written by an ordinary vector
// store or an integer atomic.  DESIGN.md section 5.4.
//
// The workspace: per input line 8 (time word) + 8 (scan) + 1 (flag) = 17 bytes, 26 with a value group (8 value + 1 class); per entry
// 2 x 24 (the two sorts' ping and pong) + 1 (head) + 8 (scan) + 4 (start) + 4 (session key) = 65 bytes and 2 x 768 per 2 048 entries of
// counts and bases; with session_stats 80 more per entry (four columns, four scans, minimum and maximum).
#include <algorithm>
#include <cstdint>
#include <utility>
#include <hip/hip_runtime.h>

#include "gx_bucket_sort_dev.hpp"
#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_outcome.hpp"
#include "gx_scan.hpp"
#include "gx_sessions.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

// (of gx_bucket_sort_dev.hpp this file launches the pair sort's two kernels; the table's two are gx_bucket.hip's and gx_series.hip's)
[[maybe_unused]] const auto not_launched_here = std::make_pair(&k_bucket_flags, &k_bucket_compact);

constexpr uint32_t SESS_LINE_BLOCKS = 2048;
enum : uint32_t { SESS_T_ENTRIES = 0, SESS_T_UNSET, SESS_T_NAN, SESS_T_OR, SESS_T_AND_INV, SESS_T_MAX, SESS_T_MIN_INV, SESS_T_WORDS };
static_assert(SESS_T_WORDS <= 8, "SessionsDev's words");

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<u64>(v), d)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_sess_keys(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots, uint32_t K,
                                                   uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data, const uint4* __restrict__ gimage,
                                                   const uint4* __restrict__ simage, const uint32_t* __restrict__ slot_of, uint64_t* __restrict__ tword,
                                                   uint8_t* __restrict__ ent, int64_t* __restrict__ val, uint8_t* __restrict__ vcls, u64* __restrict__ totals) {
    __shared__ uint4 g_l[sizeof(GroupHead) >> 4];
    __shared__ uint4 s_l[sizeof(SessionsHead) >> 4];
    __shared__ u64 l_totals[SESS_T_WORDS];
    for (uint32_t q = threadIdx.x; q < (sizeof(GroupHead) >> 4); q += 256u) g_l[q] = gimage[q];
    for (uint32_t q = threadIdx.x; q < (sizeof(SessionsHead) >> 4); q += 256u) s_l[q] = simage[q];
    if (threadIdx.x < SESS_T_WORDS) l_totals[threadIdx.x] = 0ull;
    __syncthreads();
    const GroupHead* gh = reinterpret_cast<const GroupHead*>(g_l);
    const SessionsHead* sh = reinterpret_cast<const SessionsHead*>(s_l);
    const uint32_t n_ext = gh->n_parts;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t_ent = 0, t_unset = 0, t_nan = 0;   // (the same in every lane of the wave)
    uint64_t w_or = 0, w_andi = 0, w_max = 0, w_mini = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        const uint32_t kslot = valid ? slot_of[i] : GROUP_NONE;
        const bool keyed = kslot != GROUP_NONE;   // (the line counts and its key pair is set: the build found it so)
        uint32_t why = 0u;    // of a keyed line -- 0: an entry, 1: number unset, 2: no number
        uint32_t cls = 3u;    // the value -- 0: a number, 1: unset, 2: no number, 3: the line has no value to measure
        int64_t num = 0, v = 0;
        if (keyed) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            const uint32_t e = where_find(gh->ext, n_ext, oc);
            const int32_t ng = e < n_ext ? sh->number[e] : SESSIONS_NO_NUMBER;   // (e < n_ext: a keyed line's outcome has a part)
            if (ng < 0) why = 1u;
            else {
                const uint64_t o0 = static_cast<uint64_t>(off[i]);
                const uint64_t line_units = static_cast<uint64_t>(off[i + 1]) - o0;   // (< 4 G: the build gives no key to a longer line)
                int32_t pb, pe;
                pair_of<F>(ids, caps, i, row_units, slots, static_cast<uint32_t>(ng), pb, pe);
                if (!where_pair_set(pb, pe, line_units)) why = 1u;
                else if (!number_parse_packed<NUM>(NUM ? sh->nfmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &num)) why = 2u;
                else {
                    const GroupPart part = gh->part[e];
                    if (part.value_group != GROUP_NO_VALUE) {
                        pair_of<F>(ids, caps, i, row_units, slots, part.value_group, pb, pe);
                        if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                        else cls = number_parse_packed<NUM>(NUM ? gh->fmt[e] : 0u, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                    }
                }
            }
        }
        const bool entry = keyed && why == 0u;
        if (valid) {
            ent[i] = entry ? 1 : 0;
            if (entry) {
                const uint64_t w = top_key(num, false);
                tword[i] = w;
                w_or |= w;
                w_andi |= ~w;
                w_max = umax64(w_max, w);
                w_mini = umax64(w_mini, ~w);
                if (vcls) {
                    vcls[i] = static_cast<uint8_t>(cls);
                    val[i] = cls == 0u ? v : 0;
                }
            }
        }
        t_ent += static_cast<uint64_t>(__popcll(__ballot(entry)));
        t_unset += static_cast<uint64_t>(__popcll(__ballot(keyed && why == 1u)));
        t_nan += static_cast<uint64_t>(__popcll(__ballot(keyed && why == 2u)));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        w_or |= wave_xor64(w_or, d);
        w_andi |= wave_xor64(w_andi, d);
        w_max = umax64(w_max, wave_xor64(w_max, d));
        w_mini = umax64(w_mini, wave_xor64(w_mini, d));
    }
    if (lane == 0u && t_ent) {
        atomicAdd(l_totals + SESS_T_ENTRIES, static_cast<u64>(t_ent));
        atomicOr(l_totals + SESS_T_OR, static_cast<u64>(w_or));
        atomicOr(l_totals + SESS_T_AND_INV, static_cast<u64>(w_andi));
        atomicMax(l_totals + SESS_T_MAX, static_cast<u64>(w_max));
        atomicMax(l_totals + SESS_T_MIN_INV, static_cast<u64>(w_mini));
    }
    if (lane == 0u && t_unset) atomicAdd(l_totals + SESS_T_UNSET, static_cast<u64>(t_unset));
    if (lane == 0u && t_nan) atomicAdd(l_totals + SESS_T_NAN, static_cast<u64>(t_nan));
    __syncthreads();
    if (threadIdx.x < SESS_T_WORDS && l_totals[threadIdx.x]) {
        const uint32_t q = threadIdx.x;
        if (q == SESS_T_OR || q == SESS_T_AND_INV) atomicOr(totals + q, l_totals[q]);
        else if (q == SESS_T_MAX || q == SESS_T_MIN_INV) atomicMax(totals + q, l_totals[q]);
        else atomicAdd(totals + q, l_totals[q]);
    }
}

// word[at], line[at] = line i's time word and i, at = the entries before line i; m: the entries the host read from the same scan
__global__ void __launch_bounds__(256) k_sess_compact(uint64_t n, const uint8_t* __restrict__ ent, const uint64_t* __restrict__ before,
                                                      const uint64_t* __restrict__ tword, uint32_t m, uint64_t* __restrict__ word, uint32_t* __restrict__ line) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!ent[i]) continue;
        const uint64_t at = before[i];
        if (at >= m) continue;   // (it is not: the scan counted these very flags, and the host read m from it)
        word[at] = tword[i];
        line[at] = static_cast<uint32_t>(i);
    }
}

// kword[p], pos[p] = the key number of the line at place p of the time order, and p.  A key's number is idx_off[its first line]:
// what launch_group_emit writes to keynum[] of the slot.
__global__ void __launch_bounds__(256) k_sess_number(const uint32_t* __restrict__ line, uint32_t m, uint64_t n, const uint32_t* __restrict__ slot_of,
                                                     uint32_t n_slots, const u64* __restrict__ gw, const uint64_t* __restrict__ idx_off,
                                                     uint64_t* __restrict__ kword, uint32_t* __restrict__ pos) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < m; p += stride) {
        const uint32_t i = line[p];
        uint64_t j = 0;
        if (i < n) {   // (it is: a line number of the batch)
            const uint32_t slot = slot_of[i];
            if (slot < n_slots) {   // (it is: an entry has a key)
                const uint32_t first = group_first_line(gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_FIRST]);
                if (first < n) j = idx_off[first];
            }
        }
        kword[p] = j;
        pos[p] = p;
    }
}

// One lane per entry e of the (key, time, line) order: kword[e] its key number, pos[e] its place in the time order, where tword[] and
// tline[] hold its time and line.  Gathers both into etime[e] / eline[e] and, where head is asked for (gx_group_sessions), writes head[e].
__global__ void __launch_bounds__(256) k_sess_heads(const uint64_t* __restrict__ kword, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ tword,
                                                    const uint32_t* __restrict__ tline, uint32_t m, int64_t max_gap, uint64_t* __restrict__ etime,
                                                    uint32_t* __restrict__ eline, uint8_t* __restrict__ head) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        const uint32_t p = pos[e];
        if (p >= m) {   // (it is not: the places are 0 .. m - 1)
            if (head) head[e] = 1;
            etime[e] = 0ull;
            eline[e] = GROUP_NONE;
            continue;
        }
        const uint64_t w = tword[p];
        if (head) {
            bool h = true;
            if (e > 0u) {
                const uint32_t pp = pos[e - 1u];
                const uint64_t pw = pp < m ? tword[pp] : 0ull;
                h = session_head(false, static_cast<uint32_t>(kword[e - 1u]), static_cast<uint32_t>(kword[e]), pw, w, max_gap);
            }
            head[e] = h ? 1 : 0;
        }
        etime[e] = w;
        eline[e] = tline[p];
    }
}

// start[s] = the first entry of session s; start[sbefore[m]] = m
__global__ void __launch_bounds__(256) k_sess_starts(const uint8_t* __restrict__ head, const uint64_t* __restrict__ sbefore, uint32_t m, uint32_t* __restrict__ start) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        if (!head[e]) continue;
        const uint64_t s = sbefore[e];
        if (s < m) start[s] = e;   // (it is: at most e heads lie before entry e)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t ns = sbefore[m];
        if (ns <= m) start[ns] = m;
    }
}

// One lane per session: the most entries and the longest duration, and the number of sessions for the host.
__global__ void __launch_bounds__(256) k_sess_longest(const uint32_t* __restrict__ start, const uint64_t* __restrict__ sbefore, const uint64_t* __restrict__ etime,
                                                      uint32_t m, SessionsDev2* __restrict__ dev2) {
    __shared__ u64 l_max[2];
    if (threadIdx.x < 2u) l_max[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t ns64 = sbefore[m];
    const uint32_t ns = ns64 <= m ? static_cast<uint32_t>(ns64) : 0u;   // (it is: every session has an entry)
    uint64_t lines = 0, dur = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < ns; s += stride) {
        const uint32_t b = start[s], e = start[s + 1u];
        if (b >= e || e > m) continue;   // (it is not: the starts ascend)
        lines = umax64(lines, static_cast<uint64_t>(e - b));
        dur = umax64(dur, session_gap_of(etime[b], etime[e - 1u]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lines = umax64(lines, wave_xor64(lines, d));
        dur = umax64(dur, wave_xor64(dur, d));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (lines) atomicMax(l_max + 0, static_cast<u64>(lines));
        if (dur) atomicMax(l_max + 1, static_cast<u64>(dur));
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (l_max[0]) atomicMax(reinterpret_cast<u64*>(&dev2->longest_lines), l_max[0]);
        if (l_max[1]) atomicMax(reinterpret_cast<u64*>(&dev2->longest_duration), l_max[1]);
        if (blockIdx.x == 0) dev2->n_sessions = ns64;
    }
}

// One lane per entry e, a wave over 64 consecutive entries: the columns for the four scans, and the minimum and maximum of the values
// per run of equal session number inside the wave, merged into smin[s] / smax[s] (zeroed; group_min_word / group_max_word).  head ==
// nullptr (gx_group_windows, whose sums are over windows and not over sessions): the columns alone.
__global__ void __launch_bounds__(256) k_sess_values(const uint32_t* __restrict__ eline, const uint8_t* __restrict__ head, const uint64_t* __restrict__ sbefore,
                                                     uint32_t m, uint64_t n, const int64_t* __restrict__ val, const uint8_t* __restrict__ vcls,
                                                     uint64_t* __restrict__ c_counts, uint64_t* __restrict__ c_nan, uint64_t* __restrict__ c_lo,
                                                     uint64_t* __restrict__ c_hi, u64* __restrict__ smin, u64* __restrict__ smax) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e0 = blockIdx.x * 256u + (threadIdx.x & ~63u); e0 < m; e0 += stride) {
        const uint32_t e = e0 + lane;
        const bool valid = e < m;
        uint32_t cls = 3u;
        int64_t v = 0;
        uint64_t s = ~0ull;
        if (valid) {
            const uint32_t i = eline[e];
            if (i < n) {   // (it is: a line number of the batch)
                cls = vcls[i];
                v = val[i];
            }
            if (head) s = session_of(sbefore[e], head[e] != 0);
            c_counts[e] = (cls == 0u ? 1ull : 0ull) | (cls == 1u ? (1ull << 32) : 0ull);
            c_nan[e] = cls == 2u ? 1ull : 0ull;
            c_lo[e] = cls == 0u ? (static_cast<uint64_t>(v) & 0xFFFFFFFFull) : 0ull;
            c_hi[e] = cls == 0u ? static_cast<uint64_t>(stats_high(v)) : 0ull;   // (two's complement: adds as unsigned)
        }
        if (!head) continue;   // (the same in every lane)
        // the maxima over the run of equal s that ends at this lane (the session numbers ascend along the wave); 0, "no number", is the
        // identity of the maximum, and group_stats_out looks at a word only where the session has a number
        uint64_t a = cls == 0u ? group_min_word(v) : 0ull, b = cls == 0u ? group_max_word(v) : 0ull;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t os = static_cast<uint64_t>(__shfl_up(static_cast<u64>(s), d));
            const uint64_t oa = static_cast<uint64_t>(__shfl_up(static_cast<u64>(a), d)), ob = static_cast<uint64_t>(__shfl_up(static_cast<u64>(b), d));
            if (lane >= static_cast<uint32_t>(d) && os == s) {
                a = umax64(a, oa);
                b = umax64(b, ob);
            }
        }
        const uint64_t next_s = static_cast<uint64_t>(__shfl_down(static_cast<u64>(s), 1));
        const bool run_last = valid && (lane == 63u || next_s != s);
        if (run_last && s < m) {   // (s < m: a session number)
            if (a) atomicMax(smin + s, static_cast<u64>(a));
            if (b) atomicMax(smax + s, static_cast<u64>(b));
        }
    }
}

// One lane per session s < ns (the host has checked ns against the capacities).
__global__ void __launch_bounds__(256) k_sess_emit(const uint32_t* __restrict__ start, const uint64_t* __restrict__ kword, const uint64_t* __restrict__ etime,
                                                   const uint32_t* __restrict__ eline, uint32_t m, uint32_t ns, const uint64_t* __restrict__ p_counts,
                                                   const uint64_t* __restrict__ p_nan, const uint64_t* __restrict__ p_lo, const uint64_t* __restrict__ p_hi,
                                                   const u64* __restrict__ smin, const u64* __restrict__ smax,
                                                   uint32_t* __restrict__ skey, SessionsOut out) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < ns; s += stride) {
        const uint32_t b = start[s], e = start[s + 1u];
        if (b >= e || e > m) continue;   // (it is not: the starts ascend and end at m)
        const uint32_t key = static_cast<uint32_t>(kword[b]);
        skey[s] = key;
        if (out.session_key) out.session_key[s] = key;
        if (out.session_begin) out.session_begin[s] = top_value(etime[b], false);
        if (out.session_end) out.session_end[s] = top_value(etime[e - 1u], false);
        if (out.session_first_line) out.session_first_line[s] = eline[b];
        if (out.session_lines) out.session_lines[s] = static_cast<uint64_t>(e - b);
        if (out.session_entry_begin) out.session_entry_begin[s] = b;
        if (out.session_stats && p_counts) {
            const uint64_t c = p_counts[e] - p_counts[b];
            uint64_t w[GROUP_STATS_WORDS], st[8];
            w[GROUP_S_NUMBERS] = c & 0xFFFFFFFFull;
            w[GROUP_S_UNSET] = c >> 32;
            w[GROUP_S_NOT_NUMBERS] = p_nan[e] - p_nan[b];
            w[GROUP_S_MIN] = smin[s];
            w[GROUP_S_MAX] = smax[s];
            w[GROUP_S_LO] = p_lo[e] - p_lo[b];
            w[GROUP_S_HI] = p_hi[e] - p_hi[b];
            w[GROUP_S_SPARE] = 0ull;
            group_stats_out(w, st);
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) out.session_stats[static_cast<uint64_t>(s) * 8u + q] = st[q];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.session_entry_begin) out.session_entry_begin[ns] = m;
}

// One lane per key j in 0 .. n_keys: where key j's sessions begin among the ns sessions; [n_keys] = ns.
__global__ void __launch_bounds__(256) k_sess_bounds(const uint32_t* __restrict__ skey, uint64_t ns, uint64_t n_keys, uint64_t* __restrict__ key_session_begin) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > n_keys) return;
    key_session_begin[j] = by_key_begin(skey, ns, j);
}

// One lane per entry: entry_line[e], and line_session[its line] = its session (behind a fill with "none").
__global__ void __launch_bounds__(256) k_sess_lines(const uint32_t* __restrict__ eline, const uint8_t* __restrict__ head, const uint64_t* __restrict__ sbefore,
                                                    uint32_t m, uint64_t n, uint32_t* __restrict__ entry_line, uint32_t* __restrict__ line_session) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        const uint32_t i = eline[e];
        if (entry_line) entry_line[e] = i;
        if (line_session && i < n) line_session[i] = static_cast<uint32_t>(session_of(sbefore[e], head[e] != 0));   // (i < n: a line of the batch)
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_keys_as(RowFormat fmt, unsigned blocks, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off, const GroupArgs& a,
                    const void* sessions_image, const GroupWs& g, const SessionsWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *gi = static_cast<const uint4*>(a.image), *si = static_cast<const uint4*>(sessions_image);
    u64* totals = reinterpret_cast<u64*>(w.dev);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_sess_keys<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tword, w.ent, w.val, w.vcls, totals);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_sess_keys<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tword, w.ent, w.val, w.vcls, totals);
    else
        hipLaunchKernelGGL((k_sess_keys<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), 0, stream, ids, a.caps, row_units, a.slots, K, n, o, d, gi, si, g.slot_of,
                           w.tword, w.ent, w.val, w.vcls, totals);
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
unsigned line_blocks(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, SESS_LINE_BLOCKS)); }

// the sort of the m pairs in s.word[0] / s.slot[0] by the given digits; returns the buffer that holds the result
hipError_t sort_pairs(const BucketSortWs& s, uint32_t m32, const uint8_t* digits, uint32_t n_digits, hipStream_t stream, uint32_t* result) {
    const uint64_t blocks64 = sort_blocks(m32);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    uint32_t cur = 0;
    for (uint32_t p = 0; p < n_digits; ++p) {
        const uint32_t d = digits[p];
        if (d >= BUCKET_MAX_DIGITS) return hipErrorInvalidValue;
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

SessionsWs sessions_workspace(void* ws, uint64_t n, bool values) {
    SessionsWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.image = take(sizeof(SessionsHead));
    w.dev = take(sizeof(SessionsDev));
    w.tword = reinterpret_cast<uint64_t*>(take(n * 8));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(n)));
    w.val = values ? reinterpret_cast<int64_t*>(take(n * 8)) : nullptr;
    w.ent = take(n);
    w.vcls = values ? take(n) : nullptr;
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t sessions_workspace_bytes(uint64_t n, bool values) { return sessions_workspace(nullptr, n, values).bytes; }

SessionsSortWs sessions_sort_workspace(void* ws, uint64_t m, bool stats) {
    SessionsSortWs s{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    s.dev2 = take(sizeof(SessionsDev2));
    s.by_time = bucket_sort_workspace(take(bucket_sort_workspace_bytes(m)), m);
    s.by_key = bucket_sort_workspace(take(bucket_sort_workspace_bytes(m)), m);
    s.sbefore = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
    s.sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(m + 1)));
    s.start = reinterpret_cast<uint32_t*>(take((m + 1) * 4));
    s.skey = reinterpret_cast<uint32_t*>(take(m * 4));
    s.head = take(m);
    if (stats) {
        for (int q = 0; q < 4; ++q) s.col[q] = reinterpret_cast<uint64_t*>(take(m * 8));
        for (int q = 0; q < 4; ++q) s.pre[q] = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
        s.smin = reinterpret_cast<uint64_t*>(take(m * 16));
        s.smax = s.smin + m;
    }
    s.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return s;
}
size_t sessions_sort_workspace_bytes(uint64_t m, bool stats) { return sessions_sort_workspace(nullptr, m, stats).bytes; }

// The keys pass and the scan on `stream`, n > 0 and parts > 0, behind launch_group_build: leaves SessionsDev at w.dev and w.before[n] =
// the entries.  a.image (GroupHead) and w.image (SessionsHead) are on the device.
hipError_t launch_sessions_keys(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                bool formats, const GroupWs& g, const SessionsWs& w, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(w.dev, 0, sizeof(SessionsDev), stream);
    if (e != hipSuccess) return e;
    const unsigned blocks = line_blocks(n);
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (formats) launch_keys_as<OFF, UNIT, true>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w.image, g, w);
        else launch_keys_as<OFF, UNIT, false>(fmt, blocks, stream, ids, row_units, K, n, offsets, a, w.image, g, w);
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
    return launch_exclusive_scan<uint8_t>(w.ent, n, w.sums, w.before, stream);
}

// Behind launch_sessions_keys and the host's read of SessionsDev and of n_keys on `stream`: 0 < m <= min(n, 2^30) entries, the time
// sort's plan and the key sort's digits.  The ORDER, for gx_group_sessions and gx_group_windows alike: compact, time sort, key numbers,
// key sort, and the gather of times and lines into it.  Leaves the (key, time, line) order -- key numbers in by_key.word[*key_buf],
// times and lines in by_time.word[*time_buf] / .slot[*time_buf] -- and, with head (nullptr: not wanted), head[e] under max_gap.
hipError_t launch_sessions_order(uint64_t n, uint64_t m, const SortPlan& plan, uint32_t key_digits, const GroupWs& g, const SessionsWs& w, const BucketSortWs& by_time,
                                 const BucketSortWs& by_key, int64_t max_gap, uint8_t* head, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream) {
    if (m == 0 || m > n || m > SESSIONS_MAX || plan.n_passes > SORT_MAX_PASSES || key_digits > BY_KEY_MAX_PASSES || max_gap < 0) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    hipLaunchKernelGGL(k_sess_compact, dim3(line_blocks(n)), dim3(256), 0, stream, n, w.ent, w.before, w.tword, m32, by_time.word[0], by_time.slot[0]);
    uint32_t ct = 0, ck = 0;
    hipError_t e = sort_pairs(by_time, m32, plan.digit, plan.n_passes, stream, &ct);
    if (e != hipSuccess) return e;
    const unsigned eb = line_blocks(m);
    hipLaunchKernelGGL(k_sess_number, dim3(eb), dim3(256), 0, stream, by_time.slot[ct], m32, n, g.slot_of, g.n_slots, reinterpret_cast<const u64*>(g.head_words),
                       g.idx_off, by_key.word[0], by_key.slot[0]);
    uint8_t kd[BY_KEY_MAX_PASSES];
    for (uint32_t d = 0; d < key_digits; ++d) kd[d] = static_cast<uint8_t>(d);
    e = sort_pairs(by_key, m32, kd, key_digits, stream, &ck);
    if (e != hipSuccess) return e;
    // (the time sort's other buffer is free: the entries' times and lines in the final order go there)
    hipLaunchKernelGGL(k_sess_heads, dim3(eb), dim3(256), 0, stream, by_key.word[ck], by_key.slot[ck], by_time.word[ct], by_time.slot[ct], m32, max_gap,
                       by_time.word[ct ^ 1u], by_time.slot[ct ^ 1u], head);
    *time_buf = ct ^ 1u;
    *key_buf = ck;
    return hipGetLastError();
}

// The values of the entries in the (key, time, line) order as four columns and their four scans: pre[q][e] = the sum of col[q] over the
// entries before e, for differences over any run of entries (a session, a window).  With head also the sessions' minima and maxima
// (smin / smax zeroed by the caller).  w.val / w.vcls: the keys pass', with a value group.
hipError_t launch_sessions_value_prefix(const uint32_t* eline, const uint8_t* head, const uint64_t* sbefore, uint64_t m, uint64_t n, const SessionsWs& w,
                                        uint64_t* const* col, uint64_t* const* pre, uint64_t* sums, uint64_t* smin, uint64_t* smax, hipStream_t stream) {
    if (m == 0 || m > SESSIONS_MAX || !col[0] || !w.val || !w.vcls) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sess_values, dim3(line_blocks(m)), dim3(256), 0, stream, eline, head, sbefore, static_cast<uint32_t>(m), n, w.val, w.vcls, col[0], col[1],
                       col[2], col[3], reinterpret_cast<u64*>(smin), reinterpret_cast<u64*>(smax));
    for (int q = 0; q < 4; ++q) {
        const hipError_t e = launch_exclusive_scan<uint64_t>(col[q], m, sums, pre[q], stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// Behind launch_sessions_keys and the host's read of SessionsDev and of n_keys on `stream`: the order (launch_sessions_order) with
// head[], then sbefore[], start[] and SessionsDev2 at s.dev2.
hipError_t launch_sessions_sort(uint64_t n, uint64_t m, const SortPlan& plan, uint32_t key_digits, int64_t max_gap, const GroupWs& g, const SessionsWs& w,
                                const SessionsSortWs& s, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream) {
    if (m == 0 || m > n || m > SESSIONS_MAX) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    hipError_t e = hipMemsetAsync(s.dev2, 0, sizeof(SessionsDev2), stream);
    if (e != hipSuccess) return e;
    uint32_t tb = 0, ck = 0;
    e = launch_sessions_order(n, m, plan, key_digits, g, w, s.by_time, s.by_key, max_gap, s.head, &tb, &ck, stream);
    if (e != hipSuccess) return e;
    const uint32_t ct = tb ^ 1u;
    const unsigned eb = line_blocks(m);
    e = launch_exclusive_scan<uint8_t>(s.head, m, s.sums, s.sbefore, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sess_starts, dim3(eb), dim3(256), 0, stream, s.head, s.sbefore, m32, s.start);
    hipLaunchKernelGGL(k_sess_longest, dim3(eb), dim3(256), 0, stream, s.start, s.sbefore, s.by_time.word[ct ^ 1u], m32, reinterpret_cast<SessionsDev2*>(s.dev2));
    *time_buf = ct ^ 1u;
    *key_buf = ck;
    return hipGetLastError();
}

// Behind launch_sessions_sort and the host's read of SessionsDev2 and check of the capacities: ns sessions (0 < ns <= m), n_keys keys.
// time_buf / key_buf: what launch_sessions_sort left.  out.session_stats needs a workspace made with stats and w.val / w.vcls.
hipError_t launch_sessions_emit(uint64_t n, uint64_t m, uint64_t ns, uint64_t n_keys, const SessionsWs& w, const SessionsSortWs& s, uint32_t time_buf, uint32_t key_buf,
                                const SessionsOut& out, hipStream_t stream) {
    if (m == 0 || m > SESSIONS_MAX || ns == 0 || ns > m || time_buf > 1u || key_buf > 1u) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m), ns32 = static_cast<uint32_t>(ns);
    const uint64_t* etime = s.by_time.word[time_buf];
    const uint32_t* eline = s.by_time.slot[time_buf];
    const unsigned eb = line_blocks(m);
    const bool stats = out.session_stats != nullptr;
    if (stats) {
        if (!s.col[0] || !w.val || !w.vcls) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(s.smin, 0, m * 16, stream);
        if (e != hipSuccess) return e;
        e = launch_sessions_value_prefix(eline, s.head, s.sbefore, m, n, w, s.col, s.pre, s.sums, s.smin, s.smax, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sess_emit, dim3(line_blocks(ns)), dim3(256), 0, stream, s.start, s.by_key.word[key_buf], etime, eline, m32, ns32,
                       stats ? s.pre[0] : nullptr, stats ? s.pre[1] : nullptr, stats ? s.pre[2] : nullptr, stats ? s.pre[3] : nullptr,
                       reinterpret_cast<const u64*>(s.smin), reinterpret_cast<const u64*>(s.smax), s.skey, out);
    if (out.key_session_begin)
        hipLaunchKernelGGL(k_sess_bounds, dim3(static_cast<unsigned>((n_keys + 1 + 255) / 256)), dim3(256), 0, stream, s.skey, ns, n_keys, out.key_session_begin);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!out.entry_line && !out.line_session)) return e;
    if (out.line_session) {
        e = hipMemsetAsync(out.line_session, 0xFF, n * 4, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sess_lines, dim3(eb), dim3(256), 0, stream, eline, s.head, s.sbefore, m32, n, out.entry_line, out.line_session);
    return hipGetLastError();
}

}  // namespace gx
