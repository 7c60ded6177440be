// gx_sessions.hpp -- the rule of gx_group_sessions, once: plain C++ for the host (g++ alone: tests/cpp/sessions_test.cpp) and for the
// kernels (gx_sessions.hip).  No HIP in here.  On top of gx_group.hpp (the keys and their numbers), gx_top.hpp (top_key / top_value: a
// time as an order-preserving unsigned word), gx_sort.hpp (sort_plan: the digits of the times that differ) and gx_by_key.hpp
// (by_key_passes: the key number's digits; by_key_begin: a key's run).
//
// The reference's caller collects a request's, a user's or a connection's lines right behind the extraction (README.md:26,63-79) and
// cuts them where the log falls silent:
//     byId.computeIfAbsent(r.asMap().get("id"), k -> new ArrayList<>()).add(r);
//     ... per id: sort by Instant.parse(ts).toEpochMilli(); a new session wherever ts - previous ts > maxGap
// -- Splunk's `transaction id maxpause=30s`, SQL's SUM(CASE WHEN ts - LAG(ts) OVER (PARTITION BY id ORDER BY ts) > gap THEN 1 ELSE 0 END).
// A PART is gx_group_lines' (extraction, key group, optional value group); beside it stands the part's NUMBER group, whose value is the
// line's TIME, parsed under its gx_number_format (-1: the part's lines have a key and no time).  A line counts, is keyed or adds to
// `unset` exactly as in gx_group_lines.  A keyed line is an ENTRY when its part has a number group, that group's capture names a value
// and the value parses; else it is number_unset (no number group, or the capture names nothing) or not_numbers (the value does not
// parse): keyed == entries + number_unset + not_numbers.
//
// ORDER AND BOUNDARIES.  A key's entries are ordered by (time ascending, input line ascending).  A SESSION begins at the key's first
// entry and at every entry whose time exceeds the previous entry's time by MORE than max_gap (>= 0, in the number's own unit).  In that
// order t >= prev, so (uint64) t - (uint64) prev is the true difference, 0 .. 2^64 - 1, and it is compared unsigned with max_gap: exact
// for every pair of int64, INT64_MIN and INT64_MAX included (their difference, 2^64 - 1, exceeds every max_gap).  Equal times never open
// a session.  The kernels hold a time as top_key(t, false) = t with the sign bit flipped; the difference of two such words is the
// difference of the times (session_gap_of).  Sessions leave ordered by (key number, begin time), entries by (key number, time, line).
//
// THE SORTS.  The entries' (time word, line) pairs, dense in line order, go through a stable LSD radix sort over the digits of the time
// words that differ (sort_plan); then (key number, place in time order) pairs go through a second stable sort over the key number's
// digits (by_key_passes).  Both sorts are gx_bucket_sort_dev.hpp's: ranks from ballots.  The result is ordered by (key, time, line).
//
// Not in scope: a cap on a session's span (maxspan), start / end markers (startswith), carrying unstamped lines into a session (compose
// with gx_sort_lines' carry later), the sessions' text as a new CSR batch (compose entry_line with the existing copy later), quantiles of
// durations, ranking sessions.
#pragma once
#include <cstdint>

#include "gx_by_key.hpp"
#include "gx_group.hpp"
#include "gx_sort.hpp"
#include "gx_top.hpp"

namespace gx {

constexpr uint64_t SESSIONS_MAX = GROUP_MAX_KEYS;      // max_sessions and the entries <= 2^30: what the pair sort's kernels state
constexpr int32_t SESSIONS_NO_NUMBER = -1;             // SessionsHead::number of a part whose lines have a key and no time

// prev <= t in the order of int64: the true difference, 0 .. 2^64 - 1
GX_WHERE_HD uint64_t session_gap(int64_t prev, int64_t t) { return static_cast<uint64_t>(t) - static_cast<uint64_t>(prev); }
// the same from the order-preserving words: (t ^ 2^63) - (prev ^ 2^63) == t - prev modulo 2^64
GX_WHERE_HD uint64_t session_gap_of(uint64_t prev_word, uint64_t word) { return word - prev_word; }
// does a gap open a session?  max_gap >= 0
GX_WHERE_HD bool session_opens(uint64_t gap, int64_t max_gap) { return gap > static_cast<uint64_t>(max_gap); }
// entry e of the (key, time, line) order begins a session: it is the order's first, its key differs from the entry before it, or the gap
GX_WHERE_HD bool session_head(bool first, uint32_t prev_key, uint32_t key, uint64_t prev_word, uint64_t word, int64_t max_gap) {
    return first || prev_key != key || session_opens(session_gap_of(prev_word, word), max_gap);
}
// before[e] = the heads among the entries before e (an exclusive scan of the head flags): entry e's session
GX_WHERE_HD uint64_t session_of(uint64_t before, bool head) { return head ? before : before - 1u; }   // (a non-head has a head before it)

// the time sort's plan (gx_sort.hpp's, over the entries' time words) and the key sort's number of digits from the lowest
GX_WHERE_HD SortPlan sessions_time_plan(uint64_t time_or, uint64_t time_and, uint64_t m, bool all_digits) { return sort_plan(time_or, time_and, m, all_digits); }
GX_WHERE_HD uint32_t sessions_key_digits(uint64_t n_keys, bool all_digits) { return by_key_passes(n_keys, all_digits); }

// What the sessions add to GroupHead, copied to LDS behind it: per entry of GroupHead::ext[] the number group and its packed format.
struct SessionsHead {
    uint32_t formats;                  // != 0: some nfmt[] is not LONG
    uint32_t spare[3];
    int32_t number[GROUP_MAX_PARTS];   // SESSIONS_NO_NUMBER: none
    uint8_t nfmt[GROUP_MAX_PARTS];     // number[e]'s packed number format, 0 = LONG
};
static_assert(sizeof(SessionsHead) % 16 == 0, "the head is copied in 16-byte words");

// What the keys pass leaves for the host, read in the wait with the group totals.  All words start as 0 and merge by unsigned add, OR and
// maximum: and_inv is the OR of ~word (the AND is its complement), min_inv the maximum of ~word.
struct SessionsDev {
    uint64_t entries, number_unset, not_numbers, time_or, and_inv, max_word, min_inv, spare;
};
static_assert(sizeof(SessionsDev) == 64, "the host reads it from device memory as it is");
// What the passes behind the sorts leave, read in the call's second wait.
struct SessionsDev2 {
    uint64_t n_sessions, longest_lines, longest_duration, spare;
};
static_assert(sizeof(SessionsDev2) == 32, "the host reads it from device memory as it is");

}  // namespace gx
