// gx_windows.hip -- the passes of gx_group_windows / gx_text_group_windows: for every entry of a key, the key's lines within `window`
// before it, and the entries at which that count reaches a threshold, on the device.  The reference's caller does this behind the
// extraction with a deque per key (gx_windows.hpp has the loop).  The rule -- the window's predicate, the gallop, the trip's edge, the
// peak's word -- is gx_windows.hpp; parts, keys, entries and the (key, time, line) order are gx_group_sessions' and are made by its own
// passes: launch_sessions_keys before the host's first wait, launch_sessions_order behind it (gx_sessions.hip).  Nothing of the order
// is written a second time here.
//
// Behind the order, before the call's SECOND wait (launch_windows_pass):
//   lo       one lane per entry e: window_lo's gallop backwards from e and its bisection, O(log window_lines) loads; neighbouring lanes
//            read neighbouring addresses.  wl[e] = e - lo + 1, ekey[e] = its key number.
//   flags    one lane per entry, a wave over 64 consecutive entries: flag[e] = window_trips (the entry before a wave's first is read
//            from global memory like any other), and window_peak_word reduced over runs of equal key inside the wave (six shuffle
//            steps), one integer atomicMax per run into kpeak[key] (zeroed) and one per wave of the grid into the totals' word.
//            Integers only: the same bits on every run.
//   scan     tbefore[e] = the trips before entry e; tbefore[m] = the trips.
//   trips    tent[t], tkey[t] = trip t's entry and key number.
//   count    one lane per trip: the trips that are their key's first (the tripped keys); and the peak's line and key for the totals.
// The host reads WindowsDev2 in that wait and checks the capacities.  Then (launch_windows_emit):
//   values   (with entry_window_sum) launch_sessions_value_prefix: gx_sessions.hip's columns and four scans, shared as they are.
//   entries  one lane per entry: line, key, time, window_lines, the window's sum p[e + 1] - p[lo], and line_window_lines[its line]
//            behind a fill with 0.
//   trips    one lane per trip: key, line, time, entry.
//   keys     one lane per key j in 0 .. n_keys: key_entry_begin and key_trip_begin by by_key_begin, the key's peak and its line.
// No workgroup waits for another, every loop is bounded by an argument or a constant, every value is written by an ordinary vector
// store or an integer atomic.  DESIGN.md section 5.4.
//
// The workspace: per input line gx_group_sessions' (17 bytes, 26 with a value group); per entry 2 x 24 (the two sorts' ping and pong) +
// 8 (scan) + 4 x 4 (window_lines, key, trip entry, trip key) + 1 (flag) = 73 bytes and 2 x 768 per 2 048 entries of counts and bases;
// per key 8 (peak); with entry_window_sum 64 more per entry (four columns, four scans).
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_scan.hpp"
#include "gx_windows.hpp"

namespace gx {
namespace {

typedef unsigned long long u64;   // (what the 64-bit atomics and shuffles take)
constexpr uint32_t WIN_BLOCKS = 2048;

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// One lane per entry e: wl[e] = window_lines(e), ekey[e] = its key number.
__global__ void __launch_bounds__(256) k_win_lo(const uint64_t* __restrict__ kword, const uint64_t* __restrict__ etime, uint32_t m, int64_t window,
                                                uint32_t* __restrict__ wl, uint32_t* __restrict__ ekey) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        const uint32_t lo = window_lo(kword, etime, e, window);   // (every index it reads is in 0 .. e)
        wl[e] = e - lo + 1u;
        ekey[e] = static_cast<uint32_t>(kword[e]);
    }
}

// One lane per entry e, a wave over 64 consecutive entries: flag[e], and the peak words' maxima per run of equal key inside the wave.
__global__ void __launch_bounds__(256) k_win_flags(const uint32_t* __restrict__ wl, const uint32_t* __restrict__ ekey, uint32_t m, uint32_t n_keys, uint32_t threshold,
                                                   uint8_t* __restrict__ flag, u64* __restrict__ kpeak, WindowsDev2* __restrict__ dev2) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * 256u;
    uint64_t all = 0ull;   // the maximum over this lane's entries, for the totals
    for (uint32_t e0 = blockIdx.x * 256u + (threadIdx.x & ~63u); e0 < m; e0 += stride) {
        const uint32_t e = e0 + lane;
        const bool valid = e < m;
        uint32_t key = 0xFFFFFFFFu;
        uint64_t word = 0ull;   // (0 is the identity of the maximum: a peak word is never 0)
        if (valid) {
            key = ekey[e];
            const uint32_t lines = wl[e];
            const bool key_head = e == 0u || ekey[e - 1u] != key;
            flag[e] = window_trips(lines, key_head, key_head ? 0u : wl[e - 1u], threshold) ? 1 : 0;
            word = window_peak_word(lines, e);
        }
        all = umax64(all, word);
        uint64_t a = word;     // the maximum over the run of equal key that ends at this lane (the key numbers ascend along the wave)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ok = static_cast<uint32_t>(__shfl_up(static_cast<int>(key), d));
            const uint64_t oa = static_cast<uint64_t>(__shfl_up(static_cast<u64>(a), d));
            if (lane >= static_cast<uint32_t>(d) && ok == key) a = umax64(a, oa);
        }
        const uint32_t next_key = static_cast<uint32_t>(__shfl_down(static_cast<int>(key), 1));
        const bool run_last = valid && (lane == 63u || next_key != key);
        if (run_last && key < n_keys && a) atomicMax(kpeak + key, static_cast<u64>(a));   // (key < n_keys: a key number)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) all = umax64(all, static_cast<uint64_t>(__shfl_xor(static_cast<u64>(all), d)));
    if (lane == 0u && all) atomicMax(reinterpret_cast<u64*>(&dev2->peak_word), static_cast<u64>(all));
}

// tent[t], tkey[t] = the entry and key number of trip t = tbefore[e]
__global__ void __launch_bounds__(256) k_win_trips(const uint8_t* __restrict__ flag, const uint64_t* __restrict__ tbefore, const uint32_t* __restrict__ ekey, uint32_t m,
                                                   uint32_t* __restrict__ tent, uint32_t* __restrict__ tkey) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        if (!flag[e]) continue;
        const uint64_t t = tbefore[e];
        if (t >= m) continue;   // (it is not: at most e trips lie before entry e)
        tent[t] = e;
        tkey[t] = ekey[e];
    }
}

// One lane per trip: the trips that are their key's first; the number of trips and the peak's line and key for the host.
__global__ void __launch_bounds__(256) k_win_count(const uint32_t* __restrict__ tkey, const uint64_t* __restrict__ tbefore, const uint32_t* __restrict__ ekey,
                                                   const uint32_t* __restrict__ eline, uint32_t m, WindowsDev2* __restrict__ dev2) {
    const uint64_t nt64 = tbefore[m];
    const uint32_t nt = nt64 <= m ? static_cast<uint32_t>(nt64) : 0u;   // (it is: every trip is an entry)
    uint64_t firsts = 0;   // (the same in every lane of the wave)
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t t0 = blockIdx.x * 256u + (threadIdx.x & ~63u); t0 < nt; t0 += stride) {
        const uint32_t t = t0 + (threadIdx.x & 63u);
        const bool first = t < nt && (t == 0u || tkey[t - 1u] != tkey[t]);
        firsts += static_cast<uint64_t>(__popcll(__ballot(first)));
    }
    if ((threadIdx.x & 63u) == 0u && firsts) atomicAdd(reinterpret_cast<u64*>(&dev2->tripped_keys), static_cast<u64>(firsts));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dev2->n_trips = nt64;
        // (k_win_flags, an earlier kernel of the stream, has left the peak's word complete)
        const uint32_t pe = window_peak_entry(dev2->peak_word);
        if (pe < m) {   // (it is: m > 0, and the word is some entry's)
            dev2->peak_line = eline[pe];
            dev2->peak_key = ekey[pe];
        }
    }
}

// One lane per entry: the per-entry outputs, and line_window_lines[its line] (behind a fill with 0).
__global__ void __launch_bounds__(256) k_win_entries(const uint32_t* __restrict__ eline, const uint32_t* __restrict__ ekey, const uint64_t* __restrict__ etime,
                                                     const uint32_t* __restrict__ wl, uint32_t m, uint64_t n, const uint64_t* __restrict__ p_counts,
                                                     const uint64_t* __restrict__ p_lo, const uint64_t* __restrict__ p_hi, WindowsOut out) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < m; e += stride) {
        const uint32_t i = eline[e], lines = wl[e];
        if (out.entry_line) out.entry_line[e] = i;
        if (out.entry_key) out.entry_key[e] = ekey[e];
        if (out.entry_time) out.entry_time[e] = top_value(etime[e], false);
        if (out.entry_window_lines) out.entry_window_lines[e] = lines;
        if (out.line_window_lines && i < n) out.line_window_lines[i] = lines;   // (i < n: a line of the batch)
        if (out.entry_window_sum && p_counts) {
            WindowSum s{0, 0, 0, 0};
            if (lines >= 1u && lines <= e + 1u) {   // (it is: the window is [e - lines + 1, e])
                const uint32_t lo = e + 1u - lines;
                s = window_sum(p_counts[e + 1u] - p_counts[lo], p_lo[e + 1u] - p_lo[lo], p_hi[e + 1u] - p_hi[lo]);
            }
            uint64_t* o = out.entry_window_sum + static_cast<uint64_t>(e) * 4u;
            o[0] = s.numbers;
            o[1] = s.sum_lo;
            o[2] = static_cast<uint64_t>(s.sum_hi);
            o[3] = 0ull;
        }
    }
}

// One lane per trip t < nt (the host has checked nt against the capacity).
__global__ void __launch_bounds__(256) k_win_trips_out(const uint32_t* __restrict__ tent, const uint32_t* __restrict__ tkey, const uint32_t* __restrict__ eline,
                                                       const uint64_t* __restrict__ etime, uint32_t m, uint32_t nt, WindowsOut out) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < nt; t += stride) {
        const uint32_t e = tent[t];
        if (e >= m) continue;   // (it is not: an entry)
        if (out.trip_key) out.trip_key[t] = tkey[t];
        if (out.trip_line) out.trip_line[t] = eline[e];
        if (out.trip_time) out.trip_time[t] = top_value(etime[e], false);
        if (out.trip_entry) out.trip_entry[t] = e;
    }
}

// One lane per key j in 0 .. n_keys: the bounds of its entries and of its trips; for j < n_keys its peak.
__global__ void __launch_bounds__(256) k_win_keys(const uint32_t* __restrict__ ekey, uint64_t m, const uint32_t* __restrict__ tkey, uint64_t nt,
                                                  const u64* __restrict__ kpeak, const uint32_t* __restrict__ eline, uint64_t n_keys, WindowsOut out) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > n_keys) return;
    if (out.key_entry_begin) out.key_entry_begin[j] = by_key_begin(ekey, m, j);
    if (out.key_trip_begin) out.key_trip_begin[j] = by_key_begin(tkey, nt, j);
    if (j == n_keys) return;
    const uint64_t word = kpeak[j];
    const uint32_t pe = window_peak_entry(word);
    const bool has = word != 0ull && pe < m;   // (pe < m: the word is some entry's)
    if (out.key_peak_lines) out.key_peak_lines[j] = has ? window_peak_lines(word) : 0u;
    if (out.key_peak_line) out.key_peak_line[j] = has ? eline[pe] : GROUP_NONE;
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
unsigned blocks_of(uint64_t n) { return static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, WIN_BLOCKS)); }

}  // namespace

WindowsWs windows_workspace(void* ws, uint64_t m, uint64_t n_keys, bool sums) {
    WindowsWs s{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    s.dev2 = take(sizeof(WindowsDev2));
    s.by_time = bucket_sort_workspace(take(bucket_sort_workspace_bytes(m)), m);
    s.by_key = bucket_sort_workspace(take(bucket_sort_workspace_bytes(m)), m);
    s.tbefore = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
    s.sums = reinterpret_cast<uint64_t*>(take(scan_sums_bytes(m + 1)));
    s.kpeak = reinterpret_cast<uint64_t*>(take(n_keys * 8));
    s.wl = reinterpret_cast<uint32_t*>(take(m * 4));
    s.ekey = reinterpret_cast<uint32_t*>(take(m * 4));
    s.tent = reinterpret_cast<uint32_t*>(take(m * 4));
    s.tkey = reinterpret_cast<uint32_t*>(take(m * 4));
    s.flag = take(m);
    if (sums) {
        for (int q = 0; q < 4; ++q) s.col[q] = reinterpret_cast<uint64_t*>(take(m * 8));
        for (int q = 0; q < 4; ++q) s.pre[q] = reinterpret_cast<uint64_t*>(take((m + 1) * 8));
    }
    s.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return s;
}
size_t windows_workspace_bytes(uint64_t m, uint64_t n_keys, bool sums) { return windows_workspace(nullptr, m, n_keys, sums).bytes; }

// Behind launch_sessions_keys and the host's read of SessionsDev and of n_keys on `stream`: the order (launch_sessions_order, without
// heads), then wl[], flag[], the peaks, tbefore[], the trips' entries and keys, and WindowsDev2 at s.dev2.
hipError_t launch_windows_pass(uint64_t n, uint64_t m, uint64_t n_keys, const SortPlan& plan, uint32_t key_digits, int64_t window, uint32_t threshold,
                               const GroupWs& g, const SessionsWs& w, const WindowsWs& s, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream) {
    if (m == 0 || m > n || m > WINDOWS_MAX || n_keys == 0 || n_keys > GROUP_MAX_KEYS || window < 0) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    hipError_t e = hipMemsetAsync(s.dev2, 0, sizeof(WindowsDev2), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s.kpeak, 0, n_keys * 8, stream);
    if (e != hipSuccess) return e;
    uint32_t tb = 0, kb = 0;
    e = launch_sessions_order(n, m, plan, key_digits, g, w, s.by_time, s.by_key, 0, nullptr, &tb, &kb, stream);
    if (e != hipSuccess) return e;
    const uint64_t* etime = s.by_time.word[tb];
    const uint32_t* eline = s.by_time.slot[tb];
    const unsigned eb = blocks_of(m);
    WindowsDev2* dev2 = reinterpret_cast<WindowsDev2*>(s.dev2);
    hipLaunchKernelGGL(k_win_lo, dim3(eb), dim3(256), 0, stream, s.by_key.word[kb], etime, m32, window, s.wl, s.ekey);
    hipLaunchKernelGGL(k_win_flags, dim3(eb), dim3(256), 0, stream, s.wl, s.ekey, m32, static_cast<uint32_t>(n_keys), threshold, s.flag,
                       reinterpret_cast<u64*>(s.kpeak), dev2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(s.flag, m, s.sums, s.tbefore, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_win_trips, dim3(eb), dim3(256), 0, stream, s.flag, s.tbefore, s.ekey, m32, s.tent, s.tkey);
    hipLaunchKernelGGL(k_win_count, dim3(eb), dim3(256), 0, stream, s.tkey, s.tbefore, s.ekey, eline, m32, dev2);
    *time_buf = tb;
    *key_buf = kb;
    return hipGetLastError();
}

// Behind launch_windows_pass and the host's read of WindowsDev2 and check of the capacities: nt trips (0 <= nt <= m), n_keys keys.
hipError_t launch_windows_emit(uint64_t n, uint64_t m, uint64_t nt, uint64_t n_keys, const SessionsWs& w, const WindowsWs& s, uint32_t time_buf, uint32_t key_buf,
                               const WindowsOut& out, hipStream_t stream) {
    if (m == 0 || m > WINDOWS_MAX || nt > m || n_keys == 0 || time_buf > 1u || key_buf > 1u) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m), nt32 = static_cast<uint32_t>(nt);
    const uint64_t* etime = s.by_time.word[time_buf];
    const uint32_t* eline = s.by_time.slot[time_buf];
    const bool sums = out.entry_window_sum != nullptr;
    hipError_t e = hipSuccess;
    if (sums) {
        e = launch_sessions_value_prefix(eline, nullptr, nullptr, m, n, w, s.col, s.pre, s.sums, nullptr, nullptr, stream);
        if (e != hipSuccess) return e;
    }
    if (out.line_window_lines) {
        e = hipMemsetAsync(out.line_window_lines, 0, n * 4, stream);
        if (e != hipSuccess) return e;
    }
    if (out.entry_line || out.entry_key || out.entry_time || out.entry_window_lines || out.entry_window_sum || out.line_window_lines)
        hipLaunchKernelGGL(k_win_entries, dim3(blocks_of(m)), dim3(256), 0, stream, eline, s.ekey, etime, s.wl, m32, n, sums ? s.pre[0] : nullptr,
                           sums ? s.pre[2] : nullptr, sums ? s.pre[3] : nullptr, out);
    if (nt32 && (out.trip_key || out.trip_line || out.trip_time || out.trip_entry))
        hipLaunchKernelGGL(k_win_trips_out, dim3(blocks_of(nt)), dim3(256), 0, stream, s.tent, s.tkey, eline, etime, m32, nt32, out);
    if (out.key_entry_begin || out.key_trip_begin || out.key_peak_lines || out.key_peak_line)
        hipLaunchKernelGGL(k_win_keys, dim3(static_cast<unsigned>((n_keys + 1 + 255) / 256)), dim3(256), 0, stream, s.ekey, m, s.tkey, nt,
                           reinterpret_cast<const u64*>(s.kpeak), eline, n_keys, out);
    return hipGetLastError();
}

}  // namespace gx
