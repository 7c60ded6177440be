// gx_number.hpp -- how a captured value is read as a number, once: plain C++ for the host (g++ alone: tests/cpp/number_test.cpp) and
// for every kernel that parses a value (gx_where_dev.hpp, gx_stats.hip, gx_top.hip, gx_group.hip).  No HIP in here.
//
// The reference's caller reads what a line captured right behind the extraction (README.md:26,63-79), and not every value it reads
// is a plain integer:
//     Long.parseLong(r.asMap().get("timeTakenInMsec"))                                       NUMBER_LONG
//     new BigDecimal(r.asMap().get("request_time")).setScale(s, RoundingMode.DOWN).unscaledValue().longValueExact()    NUMBER_DECIMAL
//     Instant.parse(r.asMap().get("ts")).toEpochMilli()                                      NUMBER_ISO8601, scale 3
//     ZonedDateTime.parse(t, DateTimeFormatter.ofPattern("dd/MMM/yyyy:HH:mm:ss Z", Locale.ENGLISH)).toEpochSecond()    NUMBER_CLF, scale 0
// A FORMAT is {kind, scale}; it belongs to one group of one extraction (gx_set_number_format) and every call that parses that group
// as a number parses it under its format.  The value is an int64 in the format's unit: a decimal times 10^scale, an instant in
// 10^-scale seconds since 1970-01-01T00:00:00Z.  Whatever fits no grammar or lies outside int64 is no number, as for Long.parseLong.
//
// The discipline is where_parse_int64's: every loop is bounded by the value's length, nothing outside [value, value + length) is
// read, every limit is compared BEFORE the step that could pass it, and a unit above 0x7F -- a byte of UTF-8, a 16-bit unit whose
// low byte happens to be a digit -- fits no grammar.  The calendar is integer arithmetic with divisions by constants; month lengths
// and month names are immediates, not tables in memory.
//
// Differences to Java, on purpose:
//   DECIMAL   no exponent ("1e3") and no grouping; BigDecimal takes an exponent.
//   ISO8601   year 0000, a leap second (":60"), "24:00:00", a date without a time, week dates and ordinal dates are no numbers;
//             a value without a zone is read as UTC (LocalDateTime.parse(t).toInstant(ZoneOffset.UTC)); an offset is taken as
//             ZoneOffset takes it (at most 18:00).  The year has exactly four digits, 0001 .. 9999.
//   CLF       exactly "dd/Mon/yyyy:HH:mm:ss +hhmm": English month names in that case, one space, the zone required.
//   RFC 3164 stamps ("Oct 11 22:14:15") carry no year and are out of scope: no format reads them.
#pragma once
#include <cstdint>

#include "gx_where.hpp"

namespace gx {

// (the values of GX_NUMBER_* in include/gorp_hip.h)
enum NumberKind : uint32_t { NUMBER_LONG = 0, NUMBER_DECIMAL, NUMBER_ISO8601, NUMBER_CLF, NUMBER_KINDS };
constexpr uint32_t NUMBER_MAX_DECIMAL_SCALE = 18;

// LONG takes scale 0, DECIMAL 0 .. 18, the two instants 0 (seconds), 3, 6 or 9.
GX_WHERE_HD bool number_format_ok(uint32_t kind, uint32_t scale) {
    if (kind == NUMBER_LONG) return scale == 0u;
    if (kind == NUMBER_DECIMAL) return scale <= NUMBER_MAX_DECIMAL_SCALE;
    if (kind == NUMBER_ISO8601 || kind == NUMBER_CLF) return scale == 0u || scale == 3u || scale == 6u || scale == 9u;
    return false;
}

// A format in one byte, as the passes' images carry it beside the group it names: kind in bits 0 .. 1, scale in bits 2 .. 6.
// 0 is LONG: an image of zeros names the default everywhere.
GX_WHERE_HD uint8_t number_pack(uint32_t kind, uint32_t scale) { return static_cast<uint8_t>(kind | (scale << 2)); }
GX_WHERE_HD uint32_t number_kind(uint32_t packed) { return packed & 3u; }
GX_WHERE_HD uint32_t number_scale(uint32_t packed) { return (packed >> 2) & 31u; }

// ---- DECIMAL -------------------------------------------------------------------------------------------------------------------
// [+-]? ( digits+ ( '.' digits* )? | '.' digits+ ): the decimal times 10^scale, further fraction digits dropped (toward zero).  The
// magnitude is gathered unsigned over the integer digits, the first `scale` fraction digits and, where the fraction is shorter, zeros
// in their place; the limit is compared before each of these steps, as in where_parse_int64.
template <typename VP>
GX_WHERE_HD bool number_parse_decimal(uint32_t scale, VP v, uint32_t vn, int64_t* out) {
    if (vn == 0) return false;
    const uint32_t c0 = static_cast<uint32_t>(v[0]);
    const bool neg = c0 == '-';
    uint32_t j = (neg || c0 == '+') ? 1u : 0u;
    const uint64_t tens = 922337203685477580ull;
    const uint32_t last = neg ? 8u : 7u;
    uint64_t mag = 0;
    uint32_t int_digits = 0, frac_digits = 0;
    for (; j < vn; ++j, ++int_digits) {
        const uint32_t d = static_cast<uint32_t>(v[j]) - '0';
        if (d > 9u) break;
        if (mag > tens || (mag == tens && d > last)) return false;
        mag = mag * 10u + d;
    }
    if (j < vn) {
        if (static_cast<uint32_t>(v[j]) != '.') return false;
        for (++j; j < vn; ++j, ++frac_digits) {
            const uint32_t d = static_cast<uint32_t>(v[j]) - '0';
            if (d > 9u) return false;
            if (frac_digits < scale) {
                if (mag > tens || (mag == tens && d > last)) return false;
                mag = mag * 10u + d;
            }
        }
    }
    if (int_digits == 0u && frac_digits == 0u) return false;   // a bare sign, a bare point, nothing at all
    for (uint32_t q = frac_digits; q < scale; ++q) {            // (scale <= 18: a fraction shorter than the scale)
        if (mag > tens) return false;
        mag *= 10u;
    }
    *out = neg ? static_cast<int64_t>(0ull - mag) : static_cast<int64_t>(mag);
    return true;
}

// ---- the calendar --------------------------------------------------------------------------------------------------------------
// The two digits at v[at], v[at + 1] as a number (the caller has checked at + 1 < vn); `bad` gathers "one of them was no digit", so
// that a stamp's fields are read one after the other without a branch between them and refused once.
template <typename VP>
GX_WHERE_HD uint32_t number_two(VP v, uint32_t at, uint32_t& bad) {
    const uint32_t a = static_cast<uint32_t>(v[at]) - '0', b = static_cast<uint32_t>(v[at + 1u]) - '0';
    bad |= (a > 9u ? 1u : 0u) | (b > 9u ? 1u : 0u);
    return a * 10u + b;
}
template <typename VP>
GX_WHERE_HD uint32_t number_four(VP v, uint32_t at, uint32_t& bad) {
    const uint32_t hi = number_two(v, at, bad);
    return hi * 100u + number_two(v, at + 2u, bad);
}

// the month's days in the proleptic Gregorian calendar, month 1 .. 12: 30 + (an odd month up to July, an even one from August), and
// February
GX_WHERE_HD uint32_t number_month_days(uint32_t year, uint32_t month) {
    const bool leap = (year % 4u == 0u) && (year % 100u != 0u || year % 400u == 0u);
    return month == 2u ? (leap ? 29u : 28u) : 30u + ((month + (month >> 3)) & 1u);
}

// days from 1970-01-01 to year-month-day (year >= 1, a valid date): the era of 400 years, the year of the era counted from March
GX_WHERE_HD int64_t number_days_from_civil(uint32_t year, uint32_t month, uint32_t day) {
    const uint32_t y = month <= 2u ? year - 1u : year;   // (>= 0)
    const uint32_t era = y / 400u, yoe = y - era * 400u;
    const uint32_t mp = month > 2u ? month - 3u : month + 9u;
    const uint32_t doy = (153u * mp + 2u) / 5u + day - 1u;
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
    return static_cast<int64_t>(era) * 146097 + static_cast<int64_t>(doe) - 719468;
}

// What both instants end in: the fields checked, then (epoch seconds - offset) x 10^scale + frac, frac being the first `scale`
// digits of the fraction as a number.  off_minutes: the zone's magnitude, off_neg: its sign.  At scale 9 the range is tested before
// the multiply: int64 nanoseconds reach from second -9223372037 (fraction >= 145224192) to second 9223372036 (fraction <=
// 854775807).  A negative second is taken as (second + 1) and (frac - 10^scale), so that no intermediate leaves int64 either.
GX_WHERE_HD bool number_instant(uint32_t scale, uint32_t year, uint32_t month, uint32_t day, uint32_t hh, uint32_t mi, uint32_t ss, uint32_t frac,
                                uint32_t off_minutes, bool off_neg, int64_t* out) {
    if (year < 1u || month < 1u || month > 12u || day < 1u || hh > 23u || mi > 59u || ss > 59u || off_minutes > 18u * 60u) return false;
    if (day > number_month_days(year, month)) return false;
    const int64_t off = static_cast<int64_t>(off_minutes) * 60;
    int64_t sec = number_days_from_civil(year, month, day) * 86400 + static_cast<int64_t>(hh * 3600u + mi * 60u + ss) - (off_neg ? -off : off);
    const int64_t unit = scale == 0u ? 1 : scale == 3u ? 1000 : scale == 6u ? 1000000 : 1000000000;
    int64_t f = static_cast<int64_t>(frac);
    if (scale == 9u) {
        if (sec > 9223372036ll || (sec == 9223372036ll && f > 854775807)) return false;
        if (sec < -9223372037ll || (sec == -9223372037ll && f < 145224192)) return false;
    }
    if (sec < 0) { sec += 1; f -= unit; }
    *out = sec * unit + f;
    return true;
}

// a zone's "hh" and "mm" as minutes; hours above 18 and minutes above 59 are refused here, 18:01 by number_instant
template <typename VP>
GX_WHERE_HD bool number_zone(VP v, uint32_t at_hh, bool has_mm, uint32_t at_mm, uint32_t* minutes) {
    uint32_t bad = 0;
    const uint32_t oh = number_two(v, at_hh, bad), om = has_mm ? number_two(v, at_mm, bad) : 0u;
    *minutes = oh * 60u + om;
    return bad == 0u && oh <= 18u && om <= 59u;
}

// ---- ISO8601 -------------------------------------------------------------------------------------------------------------------
// YYYY-MM-DD sep hh:mm:ss frac? zone?   sep: 'T', 't' or one space; frac: '.' or ',' and 1 .. 9 digits; zone: nothing (UTC), 'Z', 'z',
// +hh:mm, +hhmm or +hh (either sign).
template <typename VP>
GX_WHERE_HD bool number_parse_iso8601(uint32_t scale, VP v, uint32_t vn, int64_t* out) {
    if (vn < 19u) return false;
    uint32_t bad = 0;
    const uint32_t year = number_four(v, 0u, bad), month = number_two(v, 5u, bad), day = number_two(v, 8u, bad), hh = number_two(v, 11u, bad),
                   mi = number_two(v, 14u, bad), ss = number_two(v, 17u, bad);
    const uint32_t sep = static_cast<uint32_t>(v[10]);
    bool ok = bad == 0u && static_cast<uint32_t>(v[4]) == '-' && static_cast<uint32_t>(v[7]) == '-' && (sep == 'T' || sep == 't' || sep == ' ') &&
         static_cast<uint32_t>(v[13]) == ':' && static_cast<uint32_t>(v[16]) == ':';
    if (!ok) return false;
    uint32_t at = 19u, frac = 0;
    if (at < vn && (static_cast<uint32_t>(v[at]) == '.' || static_cast<uint32_t>(v[at]) == ',')) {
        ++at;
        uint32_t digits = 0;
        for (; at < vn && digits < 9u; ++at, ++digits) {   // (a tenth digit is left for the zone, which refuses it)
            const uint32_t d = static_cast<uint32_t>(v[at]) - '0';
            if (d > 9u) break;
            if (digits < scale) frac = frac * 10u + d;     // (at most nine digits: below 2^30)
        }
        if (digits == 0u) return false;
        for (uint32_t q = digits; q < scale; ++q) frac *= 10u;
    }
    const uint32_t rest = vn - at;
    uint32_t off_minutes = 0;
    bool off_neg = false;
    if (rest == 1u) {
        const uint32_t z = static_cast<uint32_t>(v[at]);
        if (z != 'Z' && z != 'z') return false;
    } else if (rest != 0u) {
        const uint32_t sign = static_cast<uint32_t>(v[at]);
        if (sign != '+' && sign != '-') return false;
        off_neg = sign == '-';
        if (rest == 3u) ok = number_zone(v, at + 1u, false, 0u, &off_minutes);
        else if (rest == 5u) ok = number_zone(v, at + 1u, true, at + 3u, &off_minutes);
        else if (rest == 6u) ok = static_cast<uint32_t>(v[at + 3u]) == ':' && number_zone(v, at + 1u, true, at + 4u, &off_minutes);
        else ok = false;
        if (!ok) return false;
    }
    return number_instant(scale, year, month, day, hh, mi, ss, frac, off_minutes, off_neg, out);
}

// ---- CLF -----------------------------------------------------------------------------------------------------------------------
// The month of three units as one packed compare against twelve immediates; 0: none (a unit above 0x7F among them included).
GX_WHERE_HD uint32_t number_clf_month(uint32_t a, uint32_t b, uint32_t c) {
    if ((a | b | c) > 0x7Fu) return 0u;
    switch ((a << 16) | (b << 8) | c) {
        case ('J' << 16) | ('a' << 8) | 'n': return 1u;
        case ('F' << 16) | ('e' << 8) | 'b': return 2u;
        case ('M' << 16) | ('a' << 8) | 'r': return 3u;
        case ('A' << 16) | ('p' << 8) | 'r': return 4u;
        case ('M' << 16) | ('a' << 8) | 'y': return 5u;
        case ('J' << 16) | ('u' << 8) | 'n': return 6u;
        case ('J' << 16) | ('u' << 8) | 'l': return 7u;
        case ('A' << 16) | ('u' << 8) | 'g': return 8u;
        case ('S' << 16) | ('e' << 8) | 'p': return 9u;
        case ('O' << 16) | ('c' << 8) | 't': return 10u;
        case ('N' << 16) | ('o' << 8) | 'v': return 11u;
        case ('D' << 16) | ('e' << 8) | 'c': return 12u;
        default: return 0u;
    }
}

// dd/Mon/yyyy:HH:mm:ss +hhmm -- 26 units, no more and no fewer
template <typename VP>
GX_WHERE_HD bool number_parse_clf(uint32_t scale, VP v, uint32_t vn, int64_t* out) {
    if (vn != 26u) return false;
    uint32_t bad = 0, off_minutes = 0;
    const uint32_t day = number_two(v, 0u, bad), year = number_four(v, 7u, bad), hh = number_two(v, 12u, bad), mi = number_two(v, 15u, bad),
                   ss = number_two(v, 18u, bad);
    const uint32_t month = number_clf_month(static_cast<uint32_t>(v[3]), static_cast<uint32_t>(v[4]), static_cast<uint32_t>(v[5]));
    const uint32_t sign = static_cast<uint32_t>(v[21]);
    const bool ok = bad == 0u && static_cast<uint32_t>(v[2]) == '/' && static_cast<uint32_t>(v[6]) == '/' && static_cast<uint32_t>(v[11]) == ':' &&
         static_cast<uint32_t>(v[14]) == ':' && static_cast<uint32_t>(v[17]) == ':' && static_cast<uint32_t>(v[20]) == ' ' && (sign == '+' || sign == '-') &&
         number_zone(v, 22u, true, 24u, &off_minutes);
    if (!ok) return false;
    return number_instant(scale, year, month, day, hh, mi, ss, 0u, off_minutes, sign == '-', out);
}

// ---- the rule ------------------------------------------------------------------------------------------------------------------
// v[0, vn) under the format {kind, scale} (number_format_ok holds; an unknown kind is no number).  LONG is where_parse_int64, bit for
// bit.
template <typename VP>
GX_WHERE_HD bool number_parse(uint32_t kind, uint32_t scale, VP v, uint32_t vn, int64_t* out) {
    if (kind == NUMBER_LONG) return where_parse_int64(v, vn, out);
    if (kind == NUMBER_DECIMAL) return number_parse_decimal(scale, v, vn, out);
    if (kind == NUMBER_ISO8601) return number_parse_iso8601(scale, v, vn, out);
    if (kind == NUMBER_CLF) return number_parse_clf(scale, v, vn, out);
    return false;
}
// ... under a packed format.  WIDE = false is the instantiation of a call whose image names LONG groups alone: the parser of today.
template <bool WIDE, typename VP>
GX_WHERE_HD bool number_parse_packed(uint32_t packed, VP v, uint32_t vn, int64_t* out) {
    if (!WIDE) return where_parse_int64(v, vn, out);
    return number_parse(number_kind(packed), number_scale(packed), v, vn, out);
}

// where_test (gx_where.hpp) with the group's format: the integer tests parse under it, everything else is unchanged.
template <bool WIDE, typename VP, typename LP>
GX_WHERE_HD bool number_where_test(uint32_t packed, uint32_t op, VP v, uint32_t vn, LP lit, uint32_t ln, int64_t number) {
    if (op == WHERE_SET) return true;
    if (op <= WHERE_CONTAINS) return where_compare(op, v, vn, lit, ln);
    int64_t value = 0;
    return number_parse_packed<WIDE>(packed, v, vn, &value) && where_int_holds(op, value, number);
}

}  // namespace gx
