// gx_where.hpp -- the rule of gx_select_lines_where, once: plain C++ for the host (g++ alone: tests/cpp/where_test.cpp) and for the
// kernel (gx_where.hip).  No HIP in here.
//
// The reference's caller tests what a line captured right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null && Long.parseLong(r.asMap().get("timeTakenInMsec")) >= 500) ...
// A TERM is one such test on one group of one extraction: test(value) XOR negate.  The value is the code units
// line[begin, end) that the group's capture offsets name; a group that is unset (Matcher.group(g) == null), or whose offsets do not
// lie inside the line (where_pair_set), fails every test.  Text tests compare code units -- bytes, or 16-bit units of a utf16 batch --
// with a literal; integer tests parse the value as Long.parseLong does for ASCII input (where_parse_int64) -- or, where the group has
// a number format of its own (gx_set_number_format), as gx_number.hpp's number_where_test does.  Every loop is bounded by the value's
// length or the literal's, and nothing outside [value, value + length) is read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GX_WHERE_HD __host__ __device__ __forceinline__
#else
#define GX_WHERE_HD inline
#endif

namespace gx {

// (the values of GX_WHERE_* in include/gorp_hip.h)
enum WhereOp : uint32_t {
    WHERE_SET = 0, WHERE_EQ, WHERE_PREFIX, WHERE_SUFFIX, WHERE_CONTAINS, WHERE_INT_EQ, WHERE_INT_LT, WHERE_INT_LE, WHERE_INT_GT, WHERE_INT_GE,
    WHERE_OPS
};
constexpr uint32_t WHERE_MAX_TERMS = 64;
constexpr uint32_t WHERE_MAX_TEXT = 255;   // code units of a literal

// A pair of capture offsets names a value when it lies inside the line's `line_units` code units; everything else is an unset group
// (-1 / -1 is what the kernels write for one; begin < 0 with end >= 0, end < begin and end beyond the line are a caller's mistake and
// are never dereferenced).
GX_WHERE_HD bool where_pair_set(int64_t begin, int64_t end, uint64_t line_units) {
    return begin >= 0 && end >= begin && static_cast<uint64_t>(end) <= line_units;
}

// n units at a == n units at b
template <typename VP, typename LP>
GX_WHERE_HD bool where_same(VP a, LP b, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j)
        if (a[j] != b[j]) return false;
    return true;
}

// WHERE_EQ .. WHERE_CONTAINS of the value v[0, vn) against the literal lit[0, ln).  An empty literal is a prefix, a suffix and a part
// of every value, and equal to the empty value alone.
template <typename VP, typename LP>
GX_WHERE_HD bool where_compare(uint32_t op, VP v, uint32_t vn, LP lit, uint32_t ln) {
    if (ln > vn) return false;
    if (op == WHERE_EQ) return ln == vn && where_same(v, lit, ln);
    if (op == WHERE_PREFIX) return where_same(v, lit, ln);
    if (op == WHERE_SUFFIX) return where_same(v + (vn - ln), lit, ln);
    // WHERE_CONTAINS: every start at which the literal still fits
    for (uint32_t at = 0; at + ln <= vn; ++at)
        if (where_same(v + at, lit, ln)) return true;
    return false;
}

// Long.parseLong for ASCII input: one optional '+' or '-', then one or more digits '0' .. '9', the value within int64 (leading zeros
// are digits like any other).  Everything else is no number: the empty value, a bare sign, any other unit, a value out of range --
// and a digit that is not ASCII, which Java takes (Character.digit): the one documented difference.  The magnitude is gathered
// unsigned and compared with the limit BEFORE each step, so nothing ever wraps.
template <typename VP>
GX_WHERE_HD bool where_parse_int64(VP v, uint32_t vn, int64_t* out) {
    if (vn == 0) return false;
    const uint32_t c0 = static_cast<uint32_t>(v[0]);
    const bool neg = c0 == '-';
    const uint32_t first = (neg || c0 == '+') ? 1u : 0u;
    if (first == vn) return false;
    // |INT64_MIN| = 9223372036854775808, INT64_MAX = 9223372036854775807: the last step may add 8 or 7 to 922337203685477580 tens
    const uint64_t tens = 922337203685477580ull;
    const uint32_t last = neg ? 8u : 7u;
    uint64_t mag = 0;
    for (uint32_t j = first; j < vn; ++j) {
        const uint32_t d = static_cast<uint32_t>(v[j]) - '0';
        if (d > 9u) return false;
        if (mag > tens || (mag == tens && d > last)) return false;
        mag = mag * 10u + d;
    }
    // (-2^63 has no positive counterpart: 0 - mag in unsigned arithmetic, then the bits as they are)
    *out = neg ? static_cast<int64_t>(0ull - mag) : static_cast<int64_t>(mag);
    return true;
}

GX_WHERE_HD bool where_int_holds(uint32_t op, int64_t value, int64_t number) {
    return op == WHERE_INT_EQ ? value == number
         : op == WHERE_INT_LT ? value < number
         : op == WHERE_INT_LE ? value <= number
         : op == WHERE_INT_GT ? value > number
                              : value >= number;
}

// One term's test on a value that is set (an unset group fails before it comes here): v[0, vn) against lit[0, ln) or `number`.
template <typename VP, typename LP>
GX_WHERE_HD bool where_test(uint32_t op, VP v, uint32_t vn, LP lit, uint32_t ln, int64_t number) {
    if (op == WHERE_SET) return true;
    if (op <= WHERE_CONTAINS) return where_compare(op, v, vn, lit, ln);
    int64_t value = 0;
    return where_parse_int64(v, vn, &value) && where_int_holds(op, value, number);
}

// The terms as the kernel reads them, built by the host (gx_api.cpp: where_image) and copied to LDS by every workgroup: the head, then
// the literals (code units of the batch, one behind the other).  The terms are ordered by extraction; ext[] holds the extractions
// that have terms, ascending, and extraction ext[e]'s terms are term[first[e] .. first[e + 1]): a lane finds its extraction's terms
// in six probes, and most lanes -- whose extraction lies outside [ext[0], ext[n_ext - 1]] -- in none.
struct WhereTerm {
    uint16_t group;
    uint16_t lit_at;    // first unit of the literal among the literals
    uint16_t lit_len;
    uint8_t op;
    uint8_t negate;
    int64_t number;
};
struct WhereHead {
    uint32_t n_terms, n_ext, lit_units;
    uint32_t formats;                      // != 0: some fmt[] is not LONG -- the host launches the pass's instantiation that reads them
    uint32_t ext[WHERE_MAX_TERMS];
    uint8_t first[WHERE_MAX_TERMS + 16];   // n_ext + 1 entries
    uint8_t fmt[WHERE_MAX_TERMS];          // term[t]'s group as a number: its packed format (gx_number.hpp), 0 = LONG; integer terms only
    WhereTerm term[WHERE_MAX_TERMS];
};
static_assert(sizeof(WhereTerm) == 16 && sizeof(WhereHead) % 16 == 0, "the head is copied in 16-byte words");

// Index of extraction k in ext[], or n_ext when it has no terms: a binary search of at most six steps (n_ext <= 64).
GX_WHERE_HD uint32_t where_find(const uint32_t* ext, uint32_t n_ext, uint32_t k) {
    uint32_t lo = 0, hi = n_ext;
    for (int s = 0; s < 7; ++s) {
        if (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ext[mid] < k) lo = mid + 1;
            else hi = mid;
        }
    }
    return lo < n_ext && ext[lo] == k ? lo : n_ext;
}

}  // namespace gx
