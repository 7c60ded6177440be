// gx_spans.hpp -- the rule of gx_group_spans, once: plain C++ for the host (g++ alone: tests/cpp/spans_test.cpp) and for the kernels
// (gx_spans.hip).  No HIP in here.  On top of gx_group.hpp (the keys and their numbers, the stats words) and gx_by_key.hpp
// (by_key_passes: the key number's digits; by_key_begin: a key's run).
//
// An application logs one line when work starts and another when it ends; two extractions capture the same id.  The reference's caller
// pairs them right behind the extraction:
//     r = gorp.extract(line);
//     if (r != null && r.name().equals("RequestStart")) { prev = open.put(id(r), r); if (prev != null) superseded.add(prev); }
//     if (r != null && r.name().equals("RequestEnd"))   { b = open.remove(id(r)); if (b == null) orphanEnds.add(r); else took.record(ts(r) - ts(b)); }
//     ... at the end: open.values() are the requests that started and never finished
// -- Splunk's `transaction id startswith=... endswith=...`.
// A PART is gx_group_lines' (extraction, key group, optional value group); beside it stand the part's NUMBER group, whose value is the
// line's TIME parsed under its gx_number_format (-1: none), and the part's ROLE, SPAN_BEGIN or SPAN_END.  A line counts, is keyed or
// adds to `unset` exactly as in gx_group_lines.  Every keyed line is an ENTRY; its role is its part's.
//
// PAIRING.  A key's entries are taken in INPUT order; time plays no part.  An END entry forms a SPAN with the entry immediately before
// it among its key's entries if and only if that entry is a BEGIN.  That one sentence is the whole rule, and it equals the put / remove
// loop above for every input: put REPLACES what was open, so only the latest begin of a key can be open, and remove EMPTIES, so behind
// an end nothing is open; what is open when an end arrives is therefore exactly "the entry before it, if that is a begin".  Every entry
// then has one STATE (span_state): 1 a span's begin, 2 a span's end, 3 a begin superseded (the next entry of its key is another begin),
// 4 a begin left open (its key's last entry), 5 an end without a begin (its key's first entry, or behind an end); 0: the line is no
// entry.  Spans leave ordered by (key number, input line of the end); a key's spans are contiguous.
//
// DURATION.  Each side's time has gx_top_lines' class -- 0 number, 1 unset (no number group, or the capture names nothing), 2 not a
// number; the span's class is the larger.  With two numbers duration = end - begin, exactly: the difference is taken in uint64, and the
// ORDER of the two times says whether it lies in int64 (span_duration).  No signed arithmetic that can overflow.  A duration outside
// int64 makes the span class 2 and counts as out_of_range; a negative one is a number like any other.
//
// THE SORT.  (key number, line) pairs, dense in line order, go through ONE stable LSD radix sort over the key number's digits
// (by_key_passes; the kernels are gx_bucket_sort_dev.hpp's): (key, line) order, in which an entry's neighbours are the entries before
// and behind it among its key's -- or another key's, which span_state is told.
//
// Not in scope: pairing in time order, roles chosen by a captured value instead of by extraction, nested or re-entrant spans (a depth
// counter), carrying open begins into the next batch (key_open_line is what a caller needs for that), the spans' text as a CSR batch,
// quantiles of durations, ranking spans.
#pragma once
#include <cstdint>

#include "gx_by_key.hpp"
#include "gx_group.hpp"

namespace gx {

constexpr uint64_t SPANS_MAX = GROUP_MAX_KEYS;   // max_spans and the entries <= 2^30: what the pair sort's kernels state
constexpr int32_t SPANS_NO_NUMBER = -1;          // SpansHead::number of a part whose lines have a key and no time
constexpr uint32_t SPAN_BEGIN = 1u, SPAN_END = 2u;   // GX_SPAN_BEGIN / GX_SPAN_END of include/gorp_hip.h
enum : uint32_t { SPAN_S_NONE = 0, SPAN_S_BEGIN, SPAN_S_END, SPAN_S_SUPERSEDED, SPAN_S_OPEN, SPAN_S_ORPHAN, SPAN_STATES };
enum : uint32_t { SPAN_C_NUMBER = 0, SPAN_C_UNSET, SPAN_C_NAN };

// The state of an entry of role `role`.  prev / next: the entry before / behind it in (key, line) order EXISTS AND HAS ITS KEY; their
// roles are looked at only then.
GX_WHERE_HD uint32_t span_state(uint32_t role, bool prev, uint32_t prev_role, bool next, uint32_t next_role) {
    if (role == SPAN_BEGIN) return !next ? SPAN_S_OPEN : next_role == SPAN_END ? SPAN_S_BEGIN : SPAN_S_SUPERSEDED;
    return prev && prev_role == SPAN_BEGIN ? SPAN_S_END : SPAN_S_ORPHAN;
}
// end - begin.  The difference modulo 2^64 is the true one when it lies in int64, and whether it does follows from the order: with
// end >= begin it is 0 .. 2^64 - 1 and fits up to 2^63 - 1; with end < begin it stands for -(2^64 - u) and fits from 2^63 on.
GX_WHERE_HD bool span_duration(int64_t begin, int64_t end, int64_t* duration) {
    const uint64_t u = static_cast<uint64_t>(end) - static_cast<uint64_t>(begin);
    const bool fits = end >= begin ? u <= 0x7FFFFFFFFFFFFFFFull : u >= 0x8000000000000000ull;
    *duration = fits ? static_cast<int64_t>(u) : 0;
    return fits;
}
GX_WHERE_HD uint32_t span_class(uint32_t begin_class, uint32_t end_class) { return begin_class > end_class ? begin_class : end_class; }

// A span as its end entry and the begin before it give it.  out_of_range: both sides were numbers and the difference left int64.
struct SpanRow {
    int64_t begin, end, duration;
    uint32_t cls;
    bool out_of_range;
};
GX_WHERE_HD SpanRow span_row(uint32_t begin_class, int64_t begin, uint32_t end_class, int64_t end) {
    SpanRow r{begin_class == SPAN_C_NUMBER ? begin : 0, end_class == SPAN_C_NUMBER ? end : 0, 0, span_class(begin_class, end_class), false};
    if (r.cls == SPAN_C_NUMBER && !span_duration(begin, end, &r.duration)) {
        r.cls = SPAN_C_NAN;
        r.out_of_range = true;
    }
    return r;
}
// a line's class and role in one byte, as the entries pass leaves them
GX_WHERE_HD uint8_t span_pack(uint32_t cls, uint32_t role) { return static_cast<uint8_t>(cls | (role << 2)); }
GX_WHERE_HD uint32_t span_pack_class(uint8_t b) { return b & 3u; }
GX_WHERE_HD uint32_t span_pack_role(uint8_t b) { return b >> 2; }

GX_WHERE_HD uint32_t spans_key_digits(uint64_t n_keys, bool all_digits) { return by_key_passes(n_keys, all_digits); }

// What the spans add to GroupHead, copied to LDS behind it: per entry of GroupHead::ext[] the number group, its packed format, the role.
struct SpansHead {
    uint32_t formats;                  // != 0: some nfmt[] is not LONG
    uint32_t spare[3];
    int32_t number[GROUP_MAX_PARTS];   // SPANS_NO_NUMBER: none
    uint8_t nfmt[GROUP_MAX_PARTS];     // number[e]'s packed number format, 0 = LONG
    uint8_t role[GROUP_MAX_PARTS];     // SPAN_BEGIN / SPAN_END
};
static_assert(sizeof(SpansHead) % 16 == 0, "the head is copied in 16-byte words");

// What the heads pass leaves, read in the call's second wait.  All words start as 0 and merge by unsigned add and maximum: state[s] the
// entries of state s, min_word / max_word group_min_word / group_max_word of the durations (0: none).
struct SpansDev {
    uint64_t state[SPAN_STATES];
    uint64_t min_word, max_word;
};
static_assert(sizeof(SpansDev) == 64, "the host reads it from device memory as it is");

}  // namespace gx
