// gx_utf8.hpp -- the UTF-8 decoding rule, once: plain C++ for the host (g++ alone: tests/cpp/utf8_test.cpp) and for the kernels
// (gx_utf8.hip).  No HIP in here.
//
// A line is bytes [beg, end) and nothing outside it is ever looked at: a line that ends in E2 followed by a line that starts with
// 82 AC is two errors, not a euro sign.  Well-formed sequences become one UTF-16 code unit, or a surrogate pair for four-byte
// sequences; ill-formed input becomes U+FFFD per MAXIMAL SUBPART (Unicode 3.9, "U+FFFD Substitution of Maximal Subparts"; the
// WHATWG decoder) -- what CPython's bytes.decode("utf-8", "replace") gives, which is what the tests compare with.  A JDK's
// decoder (new InputStreamReader(in, "UTF-8"), new String(bytes, UTF_8)) may differ from this in the NUMBER of U+FFFD it makes of
// some ill-formed input -- encoded surrogates ED A0 80, for instance, which older JDKs replace as one unit -- never for
// well-formed input.  No BOM handling: EF BB BF is U+FEFF, as in Java.
//
// The rule is locally decidable, which is what makes it parallel: the units that START at a byte depend on that byte, the three
// before it and the three after it (as far as they lie inside the line):
//   ASCII                          1
//   lead C2-DF, E0-EF, F0-F4       1; 2 when the lead is four-byte and its whole sequence is valid and complete inside the line
//   C0, C1, F5-FF                  1
//   continuation 80-BF             0 when the nearest non-continuation byte within the three before it is a lead whose valid prefix
//                                  reaches past this byte (second byte E0: A0-BF, ED: 80-9F, F0: 90-BF, F4: 80-8F, else 80-BF;
//                                  later bytes 80-BF), else 1
// A byte is passed as an int, -1 for "outside the line".
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GX_HD __host__ __device__ __forceinline__
#else
#define GX_HD inline
#endif

namespace gx {

constexpr uint16_t UTF8_REPLACEMENT = 0xFFFDu;

GX_HD bool utf8_is_cont(int b) { return b >= 0x80 && b <= 0xBF; }
// bytes of the sequence a lead begins; 0 for everything that is no lead (ASCII, continuation, C0, C1, F5-FF, outside)
GX_HD int utf8_seq_len(int b) { return b >= 0xC2 && b <= 0xDF ? 2 : b >= 0xE0 && b <= 0xEF ? 3 : b >= 0xF0 && b <= 0xF4 ? 4 : 0; }
GX_HD bool utf8_second_ok(int lead, int b) {
    const int lo = lead == 0xE0 ? 0xA0 : lead == 0xF0 ? 0x90 : 0x80;
    const int hi = lead == 0xED ? 0x9F : lead == 0xF4 ? 0x8F : 0xBF;
    return b >= lo && b <= hi;
}

// The units that start at byte b0 (0, 1 or 2); m3 m2 m1 are the bytes before it, p1 p2 p3 those after it.  units[] receives them.
GX_HD uint32_t utf8_units_at(int m3, int m2, int m1, int b0, int p1, int p2, int p3, uint16_t (&units)[2]) {
    units[0] = UTF8_REPLACEMENT;
    units[1] = 0;
    if (b0 < 0x80) { units[0] = static_cast<uint16_t>(b0); return 1u; }
    if (b0 >= 0xC0) {
        const int need = utf8_seq_len(b0);
        if (need == 2) {
            if (utf8_is_cont(p1)) units[0] = static_cast<uint16_t>((b0 & 0x1F) << 6 | (p1 & 0x3F));
        } else if (need == 3) {
            if (utf8_second_ok(b0, p1) && utf8_is_cont(p2)) units[0] = static_cast<uint16_t>((b0 & 0x0F) << 12 | (p1 & 0x3F) << 6 | (p2 & 0x3F));
        } else if (need == 4 && utf8_second_ok(b0, p1) && utf8_is_cont(p2) && utf8_is_cont(p3)) {
            const uint32_t cp = (static_cast<uint32_t>(b0 & 0x07) << 18 | static_cast<uint32_t>(p1 & 0x3F) << 12 |
                                 static_cast<uint32_t>(p2 & 0x3F) << 6 | static_cast<uint32_t>(p3 & 0x3F)) - 0x10000u;
            units[0] = static_cast<uint16_t>(0xD800u + (cp >> 10));
            units[1] = static_cast<uint16_t>(0xDC00u + (cp & 0x3FFu));
            return 2u;
        }
        return 1u;
    }
    // a continuation byte: is it inside the valid prefix of a lead up to three bytes back?
    int lead, second, dist;
    if (!utf8_is_cont(m1)) { lead = m1; second = b0; dist = 1; }
    else if (!utf8_is_cont(m2)) { lead = m2; second = m1; dist = 2; }
    else if (!utf8_is_cont(m3)) { lead = m3; second = m2; dist = 3; }
    else return 1u;
    return utf8_seq_len(lead) > dist && utf8_second_ok(lead, second) ? 0u : 1u;
}

// Byte i of the line [beg, end) of p, -1 outside it.
GX_HD int utf8_byte_in(const uint8_t* p, int64_t beg, int64_t end, int64_t i) { return i >= beg && i < end ? static_cast<int>(p[i]) : -1; }
GX_HD uint32_t utf8_units_at(const uint8_t* p, int64_t beg, int64_t end, int64_t i, uint16_t (&units)[2]) {
    return utf8_units_at(utf8_byte_in(p, beg, end, i - 3), utf8_byte_in(p, beg, end, i - 2), utf8_byte_in(p, beg, end, i - 1), utf8_byte_in(p, beg, end, i),
                         utf8_byte_in(p, beg, end, i + 1), utf8_byte_in(p, beg, end, i + 2), utf8_byte_in(p, beg, end, i + 3), units);
}

// ---- the rule on a lane's 16-byte chunk (gx_utf8.hip: 16 lanes take a line, 256 bytes a pass; tests/cpp/utf8_lanes_test.cpp plays the
// lanes on the CPU).  A lane holds its chunk as four little-endian words and the four bytes either side of it as one word each: `prev`
// = bytes ca-4 .. ca-1, `next` = bytes ca+16 .. ca+19, of which the nearest three are used.  Inside a group they are the neighbouring
// lanes' last and first words; at the group's two edges the lane loads the bytes itself (utf8_edge_prev / utf8_edge_next), as far as
// they are the line's.  Addresses are plain integers here; load(address) reads one byte.
struct Utf8Window {
    int w[22];   // w[3 + j] is byte j of the chunk; -1 where the address lies outside the line [a0, a_end)
};
GX_HD Utf8Window utf8_make_window(const uint32_t (&d)[4], uint32_t prev, uint32_t next, uint64_t ca, uint64_t a0, uint64_t a_end) {
    Utf8Window x;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 22; ++k) {
        const uint64_t addr = ca + static_cast<uint64_t>(k) - 3u;
        uint32_t byte;
        if (k < 3) byte = (prev >> ((k + 1) * 8)) & 0xFFu;
        else if (k < 19) byte = (d[(k - 3) >> 2] >> (((k - 3) & 3) * 8)) & 0xFFu;
        else byte = (next >> ((k - 19) * 8)) & 0xFFu;
        x.w[k] = addr >= a0 && addr < a_end ? static_cast<int>(byte) : -1;
    }
    return x;
}
template <typename LOAD> GX_HD uint32_t utf8_edge_prev(LOAD&& load, uint64_t ca, uint64_t a0, uint64_t a_end) {
    uint32_t prev = 0u;
    for (uint32_t k = 1; k <= 3u; ++k)
        if (ca - k >= a0 && ca - k < a_end) prev |= static_cast<uint32_t>(load(ca - k)) << ((4u - k) * 8u);
    return prev;
}
template <typename LOAD> GX_HD uint32_t utf8_edge_next(LOAD&& load, uint64_t ca, uint64_t a_end) {
    uint32_t next = 0u;
    for (uint32_t k = 0; k < 3u; ++k)
        if (ca + 16u + k < a_end) next |= static_cast<uint32_t>(load(ca + 16u + k)) << (k * 8u);
    return next;
}
// The units that start in the chunk, in order: emit(j, q, unit) for unit q (0 or 1) of byte j.  Returns their number.
template <typename EMIT> GX_HD uint32_t utf8_chunk_units(const Utf8Window& x, EMIT&& emit) {
    uint32_t cnt = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
        if (x.w[3 + j] < 0) continue;
        uint16_t u[2];
        const uint32_t k = utf8_units_at(x.w[j], x.w[j + 1], x.w[j + 2], x.w[j + 3], x.w[j + 4], x.w[j + 5], x.w[j + 6], u);
        if (k >= 1u) emit(j, 0u, u[0]);
        if (k == 2u) emit(j, 1u, u[1]);
        cnt += k;
    }
    return cnt;
}
// a whole chunk of ASCII bytes as eight words of two units each
GX_HD void utf8_widen_ascii(const uint32_t (&d)[4], uint32_t (&pair)[8]) {
    for (int q = 0; q < 8; ++q) {
        const uint32_t two = (d[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
        pair[q] = (two & 0xFFu) | ((two & 0xFF00u) << 8);
    }
}

// One line, one thread (the host's reference of the kernels; heads and tails): the units of [beg, end) into out (nullptr: count
// alone) and, beside every unit, the byte -- from beg -- of the item it starts in (unit_byte, optional; the low half of a surrogate
// pair names the sequence's first byte).  Returns the number of units.  A unit offset u maps to unit_byte[u], and u = the count
// to end - beg.
inline uint64_t utf8_transcode_line(const uint8_t* p, int64_t beg, int64_t end, uint16_t* out, uint32_t* unit_byte) {
    uint64_t n = 0;
    for (int64_t i = beg; i < end; ++i) {
        uint16_t u[2];
        const uint32_t k = utf8_units_at(p, beg, end, i, u);
        for (uint32_t q = 0; q < k; ++q) {
            if (out) out[n] = u[q];
            if (unit_byte) unit_byte[n] = static_cast<uint32_t>(i - beg);
            ++n;
        }
    }
    return n;
}

}  // namespace gx
