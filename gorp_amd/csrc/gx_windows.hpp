// gx_windows.hpp -- the rule of gx_group_windows, once: plain C++ for the host (g++ alone: tests/cpp/windows_test.cpp) and for the
// kernels (gx_windows.hip).  No HIP in here.  On top of gx_sessions.hpp: parts, keys, entries and the (key, time, line) order are
// gx_group_sessions' and nothing of them is reinterpreted.
//
// The reference's caller keeps a deque per key right behind the extraction and asks how many of the key's lines fell within the last W:
//     Deque<Long> q = recent.computeIfAbsent(r.asMap().get("user"), k -> new ArrayDeque<>());
//     q.addLast(t);  while (t - q.peekFirst() > window) q.removeFirst();
//     if (q.size() >= threshold && !tripped.contains(user)) alert(...)
// -- Splunk's `streamstats time_window=60s count by user`, SQL's COUNT(*) OVER (PARTITION BY user ORDER BY ts RANGE BETWEEN w PRECEDING
// AND CURRENT ROW), fail2ban's findtime and maxretry.
//
// THE WINDOW.  window is an int64 >= 0 in the time's own unit.  Entry e's WINDOW is the entries f of the same key with f <= e in the
// (key, time, line) order and time(e) - time(f) <= window.  f <= e gives time(f) <= time(e), so session_gap(time(f), time(e)) is the true
// difference in uint64 and it is compared unsigned with (uint64) window: exact for every pair of int64 -- window = INT64_MAX still keeps
// INT64_MIN out of INT64_MAX's window; window = 0 is the entries of the same time up to e.  An entry of the same time and a later input
// line is NOT in e's window: the caller's loop has not seen it yet.  The window is a contiguous run [lo(e), e], lo never decreases along
// a key, and window_lines(e) = e - lo(e) + 1 >= 1.
//
// TRIPS.  threshold is a uint32; 0: no trips.  Entry e TRIPS when window_lines(e) >= threshold and e is its key's first entry or
// window_lines(e - 1) < threshold: the edge, not the level, so a key trips again after its count fell below the threshold.  With
// threshold 1 exactly the first entry of every key that has entries trips.  Trips leave ordered by (key number, time, line).
//
// PEAK.  A key's peak is the largest window_lines among its entries, its peak_line the input line of the FIRST entry in the order that
// attains it; the totals' peak is the same over all entries.  Both are maxima of window_peak_word: ties go to the smallest entry index.
//
// WINDOW SUMS.  With a value group an entry's window sum is over the window's entries whose value parsed: their count and the exact
// 128-bit sum, as differences of prefix sums over the entries (exact modulo 2^64 per column, as gx_group.hip's adds are).
//
// Not in scope: windows by number of entries (streamstats window=N), centred or leading windows, window min / max / quantiles (no
// differences of prefix sums), a trip's lines as a new CSR batch, windows over all keys together, state carried from one batch into the
// next.
#pragma once
#include <cstdint>

#include "gx_sessions.hpp"
#include "gx_stats.hpp"

namespace gx {

constexpr uint64_t WINDOWS_MAX = SESSIONS_MAX;   // max_entries, max_trips and the entries <= 2^30

// f <= e in the order, both of one key: is f in e's window?  The words are top_key(time, false); window >= 0
GX_WHERE_HD bool window_holds(uint64_t f_word, uint64_t e_word, int64_t window) { return session_gap_of(f_word, e_word) <= static_cast<uint64_t>(window); }
// the same from the times themselves (f_time <= e_time)
GX_WHERE_HD bool window_holds_times(int64_t f_time, int64_t e_time, int64_t window) { return session_gap(f_time, e_time) <= static_cast<uint64_t>(window); }

// lo(e): the first f in 0 .. e with kword[f] == kword[e] && window_holds(etime[f], etime[e]) -- over f = 0 .. e that predicate is false ..
// false true .. true, and true at f = e.  Gallops backwards from e in steps 1, 2, 4, .. until the predicate fails or f = 0, then bisects
// the last interval: O(log window_lines) loads, not O(log entries).  KP, TP: pointers or anything indexable.
template <typename KP, typename TP>
GX_WHERE_HD uint32_t window_lo(KP kword, TP etime, uint32_t e, int64_t window) {
    const uint64_t key = kword[e], w = etime[e];
    uint32_t good = e;   // the predicate holds at good ...
    uint32_t bad = 0;    // ... and, when found, fails at bad < good
    bool found = false;
    for (uint32_t step = 1u; good > 0u; step <<= 1) {   // (at most 32 steps 1, 2, 4, ..: good reaches 0 or the predicate fails)
        const uint32_t f = good > step ? good - step : 0u;
        if (kword[f] == key && window_holds(etime[f], w, window)) {
            good = f;
            if (step >= 0x80000000u) break;   // (not reached: e < 2^30)
        } else {
            bad = f;
            found = true;
            break;
        }
    }
    if (!found) return good;   // (good == 0)
    while (good - bad > 1u) {
        const uint32_t mid = bad + ((good - bad) >> 1);
        if (kword[mid] == key && window_holds(etime[mid], w, window)) good = mid;
        else bad = mid;
    }
    return good;
}

// does entry e trip?  lines = window_lines(e); prev_lines = window_lines(e - 1), looked at only where e is not its key's first
GX_WHERE_HD bool window_trips(uint32_t lines, bool key_head, uint32_t prev_lines, uint32_t threshold) {
    return threshold != 0u && lines >= threshold && (key_head || prev_lines < threshold);
}

// the word whose unsigned maximum is the peak: the most lines, then the smallest entry index.  Never 0 (lines >= 1).
GX_WHERE_HD uint64_t window_peak_word(uint32_t lines, uint32_t e) { return (static_cast<uint64_t>(lines) << 32) | static_cast<uint64_t>(~e); }
GX_WHERE_HD uint32_t window_peak_lines(uint64_t word) { return static_cast<uint32_t>(word >> 32); }
GX_WHERE_HD uint32_t window_peak_entry(uint64_t word) { return ~static_cast<uint32_t>(word); }

// a window's sum from the prefix sums' differences: numbers (the low half of the counts column), and the 128-bit sum of the low and
// high halves' columns (stats_sum128)
struct WindowSum {
    uint64_t numbers, sum_lo;
    int64_t sum_hi;
    uint64_t reserved;
};
static_assert(sizeof(WindowSum) == 32, "gx_window_sum's layout");
GX_WHERE_HD WindowSum window_sum(uint64_t counts, uint64_t lo, uint64_t hi) {
    WindowSum s{counts & 0xFFFFFFFFull, 0, 0, 0};
    stats_sum128(lo, static_cast<int64_t>(hi), &s.sum_lo, &s.sum_hi);
    return s;
}

// What the passes behind the sorts leave, read in the call's second wait.
struct WindowsDev2 {
    uint64_t n_trips, tripped_keys, peak_word;
    uint32_t peak_line, peak_key;
};
static_assert(sizeof(WindowsDev2) == 32, "the host reads it from device memory as it is");

}  // namespace gx
