"""How a captured value is read as a number (gorp_amd/csrc/gx_number.hpp, gx_set_number_format) restated in Python, for the tests of
both sides (tests/test_number_host.py: the C++ rule as a program under sanitizers and gx_parse_number; tests/test_gpu_number.py: the
kernels).  re.fullmatch for each grammar, datetime.date(y, m, d).toordinal() - 719163 for the days, Python's integers for everything
else -- decimals included: no floats, no Decimal rounding modes to trust.  A value is a sequence of code units (ints); the answer is
an int or None."""
import datetime
import re

import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
LONG, DECIMAL, ISO8601, CLF = 0, 1, 2, 3
KINDS = {"long": LONG, "decimal": DECIMAL, "iso8601": ISO8601, "clf": CLF}
MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]

_LONG = re.compile(r"[+-]?[0-9]+")
_DECIMAL = re.compile(r"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))")
_ISO = re.compile(r"([0-9]{4})-([0-9]{2})-([0-9]{2})[Tt ]([0-9]{2}):([0-9]{2}):([0-9]{2})(?:[.,]([0-9]{1,9}))?"
                  r"(?:[Zz]|([+-])([0-9]{2})(?::?([0-9]{2}))?)?")
_CLF = re.compile(r"([0-9]{2})/(%s)/([0-9]{4}):([0-9]{2}):([0-9]{2}):([0-9]{2}) ([+-])([0-9]{2})([0-9]{2})" % "|".join(MONTHS))


def format_ok(kind, scale):
    if kind == LONG:
        return scale == 0
    if kind == DECIMAL:
        return 0 <= scale <= 18
    return kind in (ISO8601, CLF) and scale in (0, 3, 6, 9)


def _in_range(v):
    return v if INT64_MIN <= v <= INT64_MAX else None


def _instant(scale, y, mo, d, hh, mi, ss, frac, sign, oh, om):
    y, mo, d, hh, mi, ss, oh, om = (int(x) for x in (y, mo, d, hh, mi, ss, oh, om))
    if y < 1 or hh > 23 or mi > 59 or ss > 59 or om > 59 or oh * 60 + om > 18 * 60:
        return None
    try:
        days = datetime.date(y, mo, d).toordinal() - 719163
    except ValueError:
        return None
    offset = (oh * 3600 + om * 60) * (-1 if sign == "-" else 1)
    seconds = days * 86400 + hh * 3600 + mi * 60 + ss - offset
    digits = (frac or "")[:scale].ljust(scale, "0")
    return _in_range(seconds * 10 ** scale + (int(digits) if digits else 0))


def parse(kind, scale, units):
    """The number of the value `units` under the format (kind, scale), or None."""
    assert format_ok(kind, scale)
    units = [int(u) for u in units]
    if any(u > 0x7F for u in units):
        return None
    text = bytes(units).decode("ascii")
    if kind == LONG:
        return _in_range(int(text)) if _LONG.fullmatch(text) else None
    if kind == DECIMAL:
        m = _DECIMAL.fullmatch(text)
        if not m:
            return None
        sign, whole, frac, bare = m.groups()
        frac = (bare if whole is None else frac or "")[:scale].ljust(scale, "0")
        magnitude = int((whole or "") + frac or "0")
        return _in_range(-magnitude if sign == "-" else magnitude)
    if kind == ISO8601:
        m = _ISO.fullmatch(text)
        if not m:
            return None
        y, mo, d, hh, mi, ss, frac, sign, oh, om = m.groups()
        return _instant(scale, y, mo, d, hh, mi, ss, frac, sign, oh or 0, om or 0)
    m = _CLF.fullmatch(text)
    if not m:
        return None
    d, mon, y, hh, mi, ss, sign, oh, om = m.groups()
    return _instant(scale, y, MONTHS.index(mon) + 1, d, hh, mi, ss, None, sign, oh, om)


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
_LAST = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]


def table():
    """[(kind, scale, bytes)]: the edges of every grammar and of int64.  What each row is comes from parse(); PINNED states some of
    them by hand."""
    t = []
    iso = lambda s, scale=0: t.append((ISO8601, scale, s))
    # every month's last day and the day after (2023: no leap year)
    for m, last in enumerate(_LAST, 1):
        iso(b"2023-%02d-%02dT12:00:00Z" % (m, last))
        iso(b"2023-%02d-%02dT12:00:00Z" % (m, last + 1))
        iso(b"2023-%02d-00T12:00:00Z" % m)
        t.append((CLF, 0, b"%02d/%s/2023:12:00:00 +0000" % (last, MONTHS[m - 1].encode())))
        t.append((CLF, 0, b"%02d/%s/2023:12:00:00 +0000" % (last + 1, MONTHS[m - 1].encode())))
    iso(b"2023-00-10T12:00:00Z")
    iso(b"2023-13-10T12:00:00Z")
    for y in (1900, 2000, 2024, 2100):
        iso(b"%04d-02-29T00:00:00Z" % y)
        iso(b"%04d-02-28T23:59:59Z" % y, 3)
        iso(b"%04d-03-01T00:00:00Z" % y)
        t.append((CLF, 3, b"29/Feb/%04d:00:00:00 +0000" % y))
    # years 0000, 0001, 9999; an instant pushed before year 1 by its offset, and one pushed beyond 9999
    iso(b"0000-01-01T00:00:00Z")
    iso(b"0000-12-31T23:59:59Z")
    iso(b"0001-01-01T00:00:00Z")
    iso(b"0001-01-01T00:00:00Z", 6)
    iso(b"9999-12-31T23:59:59Z")
    iso(b"9999-12-31T23:59:59.999999Z", 6)
    iso(b"0001-01-01T00:00:00+01:00")
    iso(b"0001-01-01T00:00:00+18:00", 3)
    iso(b"9999-12-31T23:59:59-18:00", 6)
    iso(b"10000-01-01T00:00:00Z")
    iso(b"999-01-01T00:00:00Z")
    iso(b"+2026-01-01T00:00:00Z")
    t.append((CLF, 0, b"01/Jan/0000:00:00:00 +0000"))
    t.append((CLF, 0, b"01/Jan/0001:00:00:00 +0100"))
    t.append((CLF, 6, b"31/Dec/9999:23:59:59 -1800"))
    # offsets +-18:00 and 18:01 in all three spellings; minutes of 60; odd shapes
    for sign in (b"+", b"-"):
        for z in (b"18:00", b"1800", b"18", b"18:01", b"1801", b"19", b"17:59", b"1759", b"00:00", b"0000", b"00", b"05:30", b"0530", b"05", b"05:60", b"0560",
                  b"5", b"530", b"05:3", b"05:300", b"05-30", b"0:530", b"", b"05:", b":30"):
            iso(b"2026-01-03T04:00:00" + sign + z)
            iso(b"2026-01-03T04:00:00.5" + sign + z, 3)
        for z in (b"1800", b"1801", b"1900", b"0000", b"0530", b"0560", b"18:00", b"18", b"180", b"18000", b""):
            t.append((CLF, 0, b"03/Jan/2026:04:00:00 " + sign + z))
    iso(b"2026-01-03T04:00:00ZZ")
    iso(b"2026-01-03T04:00:00Z+00")
    iso(b"2026-01-03T04:00:00 Z")
    iso(b"2026-01-03T04:00:00UTC")
    # fractions of 1, 9 and 10 digits, with ',' as well, at every scale; a bare point
    for scale in (0, 3, 6, 9):
        for frac in (b".1", b".123456789", b".1234567891", b",1", b",123456789", b",1234567891", b".", b",", b".12345", b".000000001", b".999999999", b".9995",
                     b".1a", b".-1", b";1"):
            for zone in (b"", b"Z", b"-03:00"):
                iso(b"2026-01-03T04:00:00" + frac + zone, scale)
    # :60 and 24:00:00, and their neighbours
    for clock in (b"23:59:60", b"24:00:00", b"23:60:00", b"23:59:59", b"00:00:00", b"99:99:99", b"2:00:00", b"02:0:00", b"02:00:0", b"02-00-00", b"02:00"):
        iso(b"2026-01-03T" + clock + b"Z")
        t.append((CLF, 0, b"03/Jan/2026:" + clock + b" +0000"))
    # lower-case t / z, a space, and what is no separator
    for sep in (b"T", b"t", b" ", b"  ", b"_", b"", b"\t"):
        iso(b"2026-01-03" + sep + b"04:00:00z")
        iso(b"2026-01-03" + sep + b"04:00:00", 3)
    # date-only, week dates, ordinal dates, other punctuation, the empty value
    for s in (b"2026-01-03", b"2026-W01-6T04:00:00Z", b"2026-003T04:00:00Z", b"2026/01/03T04:00:00Z", b"20260103T040000Z", b"2026-01-03T04:00Z", b"", b"T",
              b"2026-01-03T04:00:00", b"2026-1-3T04:00:00Z", b"2026-01-03T04:00:0", b" 2026-01-03T04:00:00Z", b"2026-01-03T04:00:00Z ", b"2O26-01-03T04:00:00Z"):
        iso(s)
        iso(s, 9)
    # both int64-nanosecond edge instants and one nanosecond beyond each
    for s in (b"1677-09-21T00:12:43.145224192Z", b"1677-09-21T00:12:43.145224191Z", b"2262-04-11T23:47:16.854775807Z", b"2262-04-11T23:47:16.854775808Z",
              b"1677-09-21T00:12:43Z", b"1677-09-21T00:12:44Z", b"2262-04-11T23:47:16Z", b"2262-04-11T23:47:17Z", b"1677-09-21T00:12:42.999999999Z",
              b"1677-09-21T01:12:43.145224192+01:00", b"1677-09-21T01:12:43.145224191+01:00", b"2262-04-11T22:47:16.854775807-01:00",
              b"2262-04-11T22:47:16.854775808-01:00", b"0001-01-01T00:00:00Z", b"9999-12-31T23:59:59Z"):
        for scale in (9, 6, 3, 0):
            iso(s, scale)
    t.append((CLF, 9, b"21/Sep/1677:00:12:43 +0000"))
    t.append((CLF, 9, b"21/Sep/1677:00:12:44 +0000"))
    t.append((CLF, 9, b"11/Apr/2262:23:47:16 +0000"))
    t.append((CLF, 9, b"11/Apr/2262:23:47:17 +0000"))
    # the negative-epoch floor
    for s in (b"1969-12-31T23:59:59.999Z", b"1969-12-31T23:59:59.9999Z", b"1969-12-31T23:59:59Z", b"1970-01-01T00:00:00Z", b"1970-01-01T00:00:00.0009Z",
              b"1969-12-31T23:59:59.000000001Z", b"1970-01-01T00:00:00+00:01"):
        for scale in (0, 3, 6, 9):
            iso(s, scale)
    # CLF: the shape, exactly
    for s in (b"11/Oct/2026:22:14:15 +0200", b"11/oct/2026:22:14:15 +0200", b"11/OCT/2026:22:14:15 +0200", b"11/Oct/2026:22:14:15", b"11/Oct/2026:22:14:15 ",
              b"11/Oct/2026:22:14:15  +0200", b"11/Oct/2026:22:14:15+0200", b"11/Oct/2026:22:14:15 Z", b"11/Oct/2026:22:14:15 +02:00", b"1/Oct/2026:22:14:15 +0200",
              b"11/Okt/2026:22:14:15 +0200", b"11/Oct/26:22:14:15 +0200", b"11-Oct-2026:22:14:15 +0200", b"11/Oct/2026 22:14:15 +0200", b"[11/Oct/2026:22:14:15 +0200]",
              b"11/Oct/2026:22:14:15 0200", b"11/10/2026:22:14:15 +0200", b"Oct 11 22:14:15", b"11/Sept/2026:22:14:15 +0200", b"00/Oct/2026:22:14:15 +0200",
              b"11/Oct/2026:22:14:15 -0000", b""):
        for scale in (0, 3):
            t.append((CLF, scale, s))
    for mon in MONTHS:
        t.append((CLF, 0, b"15/" + mon.encode() + b"/2026:01:02:03 -0700"))
        t.append((CLF, 0, b"15/" + mon.upper().encode() + b"/2026:01:02:03 -0700"))
        t.append((CLF, 0, b"15/" + mon[:2].encode() + b"x/2026:01:02:03 -0700"))
    # decimals
    for s in (b".5", b"5.", b".", b"+", b"-", b"", b"1e3", b"1E3", b"-0.0004", b"0.0004", b"12.7", b"-12.7", b"12.7777777777777777777777777", b"007.5", b"00000000000000000000000001.5",
              b"+.5", b"-.5", b"+5.", b"1.2.3", b"1,5", b"1_000", b"1 ", b" 1", b"--1", b"+-1", b"0", b"-0", b"-0.0", b"5", b"123456789.123456789", b"0.137", b"0.1379",
              b".000", b"..5", b"5..", b"1.5f", b"0x10", b"NaN", b"99999999999999999999", b"-99999999999999999999", b"0.99999999999999999999999999"):
        for scale in (0, 3, 18):
            t.append((DECIMAL, scale, s))
    # the int64 edges at scale 0 and at scale 18
    for s in (b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"9223372036854775807.9", b"-9223372036854775808.9",
              b"9223372036854775808.0", b"922337203685477580.7", b"922337203685477580.8", b"-922337203685477580.8", b"-922337203685477580.9"):
        t.append((DECIMAL, 0, s))
        t.append((DECIMAL, 1, s))
    for s in (b"9.223372036854775807", b"9.223372036854775808", b"-9.223372036854775808", b"-9.223372036854775809", b"9.2233720368547758079", b"-9.2233720368547758089",
              b"9.3", b"9.2", b"-9.3", b"10", b"9", b"-9", b"-10", b"9.", b"0.000000000000000001", b"-0.0000000000000000019", b"9.22337203685477581"):
        t.append((DECIMAL, 18, s))
        t.append((DECIMAL, 17, s))
    # LONG is Long.parseLong: where_oracle.INT_TABLE's values, and what only the other kinds take
    for s in (b"0", b"-0", b"+5", b"007", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"", b"-", b"12a", b"12.7",
              b"2026-01-03T04:00:00Z"):
        t.append((LONG, 0, s))
    return t


# a unit >= 0x80, and as utf16 a unit >= 0x100 whose low byte is a digit: (kind, scale, units, wide only)
def unit_cases():
    out = []
    for kind, scale, text in ((LONG, 0, b"123"), (DECIMAL, 3, b"1.25"), (DECIMAL, 3, b".5"), (ISO8601, 3, b"2026-01-03T04:00:00.123+05:30"),
                              (ISO8601, 0, b"2026-01-03T04:00:00Z"), (CLF, 0, b"11/Oct/2026:22:14:15 +0200")):
        for at in range(len(text)):
            u = list(text)
            out.append((kind, scale, u[:at] + [u[at] | 0x80] + u[at + 1:], False))
            out.append((kind, scale, u[:at] + [u[at] + 0x100] + u[at + 1:], True))
            out.append((kind, scale, u[:at] + [u[at] + 0xFF00] + u[at + 1:], True))
        out.append((kind, scale, list(text) + [0xE9], False))
        out.append((kind, scale, list(text) + [0x130], True))
    return out


# a few rows stated by hand, so that the restatement is not its own only witness
PINNED = [
    (ISO8601, 3, b"1969-12-31T23:59:59.999Z", -1),
    (ISO8601, 0, b"1970-01-01T00:00:00Z", 0),
    (ISO8601, 0, b"2026-01-03T04:00:00Z", 1767412800),
    (ISO8601, 3, b"2026-01-03T04:00:00,25+05:30", 1767393000250),
    (ISO8601, 0, b"2026-01-03 04:00:00", 1767412800),
    (ISO8601, 9, b"1677-09-21T00:12:43.145224192Z", INT64_MIN),
    (ISO8601, 9, b"1677-09-21T00:12:43.145224191Z", None),
    (ISO8601, 9, b"2262-04-11T23:47:16.854775807Z", INT64_MAX),
    (ISO8601, 9, b"2262-04-11T23:47:16.854775808Z", None),
    (ISO8601, 0, b"0001-01-01T00:00:00Z", -62135596800),
    (ISO8601, 0, b"0001-01-01T00:00:00+01:00", -62135600400),
    (ISO8601, 0, b"9999-12-31T23:59:59Z", 253402300799),
    (ISO8601, 0, b"0000-01-01T00:00:00Z", None),
    (ISO8601, 0, b"2026-01-03T23:59:60Z", None),
    (ISO8601, 0, b"2026-01-03T24:00:00Z", None),
    (ISO8601, 0, b"2026-01-03", None),
    (ISO8601, 0, b"2026-01-03T04:00:00+18:00", 1767412800 - 18 * 3600),
    (ISO8601, 0, b"2026-01-03T04:00:00+18:01", None),
    (ISO8601, 0, b"2026-01-03T04:00:00.1234567891Z", None),
    (ISO8601, 0, b"1900-02-29T00:00:00Z", None),
    (ISO8601, 0, b"2000-02-29T00:00:00Z", 951782400),
    (CLF, 0, b"11/Oct/2026:22:14:15 +0200", 1791749655),
    (CLF, 0, b"11/oct/2026:22:14:15 +0200", None),
    (CLF, 0, b"11/Oct/2026:22:14:15", None),
    (CLF, 0, b"11/Oct/2026:22:14:15  +0200", None),
    (DECIMAL, 3, b"-0.0004", 0),
    (DECIMAL, 0, b"12.7", 12),
    (LONG, 0, b"12.7", None),
    (DECIMAL, 3, b"0.137", 137),
    (DECIMAL, 3, b".5", 500),
    (DECIMAL, 3, b"5.", 5000),
    (DECIMAL, 3, b".", None),
    (DECIMAL, 3, b"+", None),
    (DECIMAL, 3, b"1e3", None),
    (DECIMAL, 18, b"9.223372036854775807", INT64_MAX),
    (DECIMAL, 18, b"9.223372036854775808", None),
    (DECIMAL, 18, b"-9.223372036854775808", INT64_MIN),
    (DECIMAL, 18, b"-9.2233720368547758089", INT64_MIN),
]


def random_values(kind, scale, count, seed):
    """Seeded values of one format, most of them numbers, the rest one edit away from one."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        if kind == LONG:
            s = b"%d" % int(rng.integers(-10 ** 6, 10 ** 6))
        elif kind == DECIMAL:
            whole = int(rng.integers(0, 10 ** int(rng.integers(1, max(2, min(12, 20 - scale))))))   # (up to the edge of int64 at this scale, now and then beyond)
            frac = b"".join(b"%d" % int(d) for d in rng.integers(0, 10, int(rng.integers(0, 8))))
            s = [b"", b"-", b"+"][int(rng.integers(0, 3))] + (b"%d" % whole if rng.integers(0, 8) else b"") + (b"." + frac if len(frac) or rng.integers(0, 2) else b"")
        else:
            # (a span that stays inside int64 nanoseconds most of the time, and leaves it now and then)
            y = int(rng.integers(1, 10000)) if rng.integers(0, 8) == 0 else int(rng.integers(1960, 2040))
            mo, d = int(rng.integers(1, 13)), int(rng.integers(1, 32))
            hh, mi, ss = int(rng.integers(0, 25)), int(rng.integers(0, 61)), int(rng.integers(0, 61))
            if rng.integers(0, 4):
                d, hh, mi, ss = min(d, 28), min(hh, 23), min(mi, 59), min(ss, 59)
            oh, om = int(rng.integers(0, 19)), int(rng.integers(0, 4)) * 15
            sign = b"+-"[int(rng.integers(0, 2)):][:1]
            if kind == CLF:
                s = b"%02d/%s/%04d:%02d:%02d:%02d %s%02d%02d" % (d, MONTHS[mo - 1].encode(), y, hh, mi, ss, sign, oh, om)
            else:
                sep = [b"T", b"t", b" "][int(rng.integers(0, 3))]
                digits = int(rng.integers(0, 10))
                frac = (b".," [int(rng.integers(0, 2)):][:1] + b"".join(b"%d" % int(x) for x in rng.integers(0, 10, digits))) if digits else b""
                zone = [b"", b"Z", b"z", sign + b"%02d:%02d" % (oh, om), sign + b"%02d%02d" % (oh, om), sign + b"%02d" % oh][int(rng.integers(0, 6))]
                s = b"%04d-%02d-%02d%s%02d:%02d:%02d%s%s" % (y, mo, d, sep, hh, mi, ss, frac, zone)
        if len(s) and rng.integers(0, 10) == 0:
            at = int(rng.integers(0, len(s)))
            s = s[:at] + [b"", b"x", b"0", b":"][int(rng.integers(0, 4))] + s[at + 1:]
        out.append(s)
    return out
