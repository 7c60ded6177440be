"""gx_set_number_format / gx_get_number_format / gx_parse_number as far as they go without a GPU: the struct, the symbols and the
constants, the round trip on a host-only handle and every refusal, the blob that does not change, the Python side's resolution of
names, kinds and string numbers -- and the rule itself: gorp_amd/csrc/gx_number.hpp, plain C++, built with g++
-fsanitize=address,undefined into tests/cpp/number_test.cpp and run as a program of its own on number_oracle's case table and on seeded
random values, as bytes and as 16-bit units, each value in a buffer of exactly its length, against number_oracle.parse.  Every verdict
and every value is compared exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import number_oracle as NO
from gorp_amd import _native as N
from gorp_amd import gorp as G
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from where_oracle import INT_OPS, holds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_set_number_format", "gx_get_number_format", "gx_parse_number"]
FORMATS = [(NO.LONG, 0), (NO.DECIMAL, 0), (NO.DECIMAL, 3), (NO.DECIMAL, 18), (NO.ISO8601, 0), (NO.ISO8601, 3), (NO.ISO8601, 6), (NO.ISO8601, 9), (NO.CLF, 0),
           (NO.CLF, 9)]


def three_rules():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),
                           FlattenedExtraction("beta", [["text", "c"]]),
                           FlattenedExtraction("gamma", [["text", "d"], ["extractor", "y", [["pattern", "\\d+"]]], ["extractor", "y", [["pattern", "x*"]]],
                                                         ["extractor", "z", [["pattern", "q?"]]]])], host_only=True)


# ---------------------------------------------------------------------------
# the restatement against rows stated by hand
# ---------------------------------------------------------------------------
def test_the_restatement_agrees_with_rows_stated_by_hand():
    for kind, scale, text, want in NO.PINNED:
        assert NO.parse(kind, scale, text) == want, (kind, scale, text)
    table = NO.table()
    assert len(table) > 800 and len(set(table)) > 800
    numbers = [NO.parse(k, s, t) for k, s, t in table]
    assert 300 < sum(v is not None for v in numbers) < len(table) - 300          # both verdicts, hundreds of times
    assert NO.INT64_MIN in numbers and NO.INT64_MAX in numbers and -1 in numbers
    for kind, scale in FORMATS:
        assert NO.format_ok(kind, scale)
        got = [NO.parse(kind, scale, v) for v in NO.random_values(kind, scale, 200, 5)]
        assert sum(v is not None for v in got) > 80, (kind, scale)               # the random values are mostly numbers ...
        assert kind == NO.LONG or sum(v is None for v in got) > 5, (kind, scale)  # ... and some are not


# ---------------------------------------------------------------------------
# struct, symbols, constants; the handle's table of formats
# ---------------------------------------------------------------------------
def test_struct_layout_symbols_and_constants():
    T = N.gx_number_format
    assert C.sizeof(T) == 8
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("kind", 0), ("scale", 4)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert [N.GX_NUMBER_LONG, N.GX_NUMBER_DECIMAL, N.GX_NUMBER_ISO8601, N.GX_NUMBER_CLF] == [0, 1, 2, 3] == [NO.LONG, NO.DECIMAL, NO.ISO8601, NO.CLF]
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    enum = header[header.index("enum { GX_NUMBER_LONG = 0"):]
    assert re.findall(r"GX_NUMBER_\w+", enum[:enum.index("}")]) == ["GX_NUMBER_LONG", "GX_NUMBER_DECIMAL", "GX_NUMBER_ISO8601", "GX_NUMBER_CLF"]
    assert "typedef struct gx_number_format { uint32_t kind, scale; } gx_number_format;" in header
    assert G.NUMBER_KINDS == ("long", "decimal", "iso8601", "clf") and {k: G.NUMBER_KINDS.index(k) for k in G.NUMBER_KINDS} == NO.KINDS
    mirror = open(os.path.join(ROOT, "include", "gorp.hpp")).read()
    assert "void setNumberFormat(" in mirror and "gx_number_format numberFormat(" in mirror


def fmt(kind, scale):
    return N.gx_number_format(kind, scale)


def get(L, h, k, g):
    out = fmt(77, 77)
    assert L.gx_get_number_format(h, k, g, C.byref(out)) == N.GX_OK
    return out.kind, out.scale


def test_set_get_reset_and_every_refusal_on_a_host_only_handle():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    h = g._h.ptr
    pairs = [(0, 0), (2, 0), (2, 1), (2, 2)]
    assert [get(L, h, k, q) for k, q in pairs] == [(0, 0)] * 4                   # a new handle: LONG everywhere
    valid = [(kind, scale) for kind in range(4) for scale in range(0, 40) if NO.format_ok(kind, scale)]
    assert len(valid) == 1 + 19 + 4 + 4
    for kind, scale in valid:
        assert L.gx_set_number_format(h, 2, 1, C.byref(fmt(kind, scale))) == N.GX_OK
        assert get(L, h, 2, 1) == (kind, scale)
        assert [get(L, h, k, q) for k, q in pairs if (k, q) != (2, 1)] == [(0, 0)] * 3   # ... of that group alone
    assert L.gx_set_number_format(h, 0, 0, C.byref(fmt(NO.CLF, 6))) == N.GX_OK
    assert L.gx_set_number_format(h, 2, 1, None) == N.GX_OK                      # NULL: back to LONG
    assert [get(L, h, k, q) for k, q in pairs] == [(NO.CLF, 6), (0, 0), (0, 0), (0, 0)]
    # GX_E_ARG: h / k / g out of range, an unknown kind, a scale the kind does not take -- and nothing changes
    assert L.gx_set_number_format(h, 2, 2, C.byref(fmt(NO.ISO8601, 3))) == N.GX_OK
    ok = fmt(NO.DECIMAL, 2)
    refused = [(None, 0, 0, ok), (h, -1, 0, ok), (h, 3, 0, ok), (h, 0, 1, ok), (h, 0, -1, ok), (h, 1, 0, ok), (h, 2, 3, ok)]
    refused += [(h, 2, 2, fmt(kind, scale)) for kind in range(4) for scale in list(range(0, 40)) + [2 ** 32 - 1] if not NO.format_ok(kind, scale)]
    refused += [(h, 2, 2, fmt(kind, 0)) for kind in (4, 5, 255, 2 ** 32 - 1)]
    for hh, k, q, f in refused:
        assert L.gx_set_number_format(hh, k, q, C.byref(f)) == N.GX_E_ARG, (k, q, f.kind, f.scale)
        assert "gx_set_number_format" in N.last_error()
    out = fmt(0, 0)
    for hh, k, q in [(None, 0, 0), (h, -1, 0), (h, 3, 0), (h, 0, 1), (h, 1, 0), (h, 2, 3), (h, 2, -1)]:
        assert L.gx_get_number_format(hh, k, q, C.byref(out)) == N.GX_E_ARG
    assert L.gx_get_number_format(h, 0, 0, None) == N.GX_E_ARG
    assert [get(L, h, k, q) for k, q in pairs] == [(NO.CLF, 6), (0, 0), (0, 0), (NO.ISO8601, 3)]


def test_the_format_is_not_part_of_the_blob():
    g = three_rules()
    before = g.blob().tobytes()
    g.set_number_format("gamma", "z", "iso8601", 9)
    g.set_number_format("alpha", "x", "decimal", 18)
    assert g.blob().tobytes() == before
    again = Gorp.from_blob(g.blob(), g._extractions, host_only=True)
    assert again.number_format("gamma", "z") == ("long", 0) and again.number_format(0, 0) == ("long", 0)
    assert again.blob().tobytes() == before
    # the C call itself: a handle from the blob starts with LONG everywhere
    L = N.lib()
    blob = np.frombuffer(before, dtype=np.uint8)
    h = C.c_void_p()
    assert L.gx_create_from_blob(blob.ctypes.data, blob.size, N.GX_CREATE_HOST_ONLY, C.byref(h)) == N.GX_OK
    try:
        assert [get(L, h, k, q) for k, q in [(0, 0), (2, 0), (2, 1), (2, 2)]] == [(0, 0)] * 4
        assert L.gx_set_number_format(h, 2, 2, C.byref(fmt(NO.CLF, 3))) == N.GX_OK and get(L, h, 2, 2) == (NO.CLF, 3)
        assert g.number_format("gamma", "z") == ("iso8601", 9)                   # (the other handle keeps its own)
    finally:
        L.gx_destroy(h)


# ---------------------------------------------------------------------------
# gx_parse_number
# ---------------------------------------------------------------------------
def c_parse(kind, scale, units, wide):
    L = N.lib()
    a = np.array(list(units), dtype=np.uint16 if wide else np.uint8)
    value, is_number = C.c_int64(-12345), C.c_int32(-1)
    f = fmt(kind, scale)
    assert L.gx_parse_number(C.byref(f), a.ctypes.data if a.size else None, a.size, 1 if wide else 0, C.byref(value), C.byref(is_number)) == N.GX_OK
    assert is_number.value in (0, 1)
    return value.value if is_number.value else None


def test_parse_number_is_the_restatement_on_the_whole_table():
    for kind, scale, text in NO.table():
        want = NO.parse(kind, scale, text)
        assert c_parse(kind, scale, text, False) == want, (kind, scale, text)
        assert c_parse(kind, scale, text, True) == want, (kind, scale, text)
    for kind, scale, units, wide in NO.unit_cases():
        assert NO.parse(kind, scale, units) is None
        assert c_parse(kind, scale, units, wide) is None, (kind, scale, units)
    for kind, scale, text, want in NO.PINNED:
        assert c_parse(kind, scale, text, False) == want
    # NULL format: LONG; refusals
    L = N.lib()
    value, is_number = C.c_int64(0), C.c_int32(0)
    a = np.frombuffer(b"-42", dtype=np.uint8)
    assert L.gx_parse_number(None, a.ctypes.data, 3, 0, C.byref(value), C.byref(is_number)) == N.GX_OK and (value.value, is_number.value) == (-42, 1)
    assert L.gx_parse_number(None, None, 0, 0, C.byref(value), C.byref(is_number)) == N.GX_OK and is_number.value == 0
    assert L.gx_parse_number(None, None, 3, 0, C.byref(value), C.byref(is_number)) == N.GX_E_ARG
    assert L.gx_parse_number(None, a.ctypes.data, 3, 0, None, C.byref(is_number)) == N.GX_E_ARG
    assert L.gx_parse_number(None, a.ctypes.data, 3, 0, C.byref(value), None) == N.GX_E_ARG
    for kind, scale in ((NO.LONG, 1), (NO.DECIMAL, 19), (NO.ISO8601, 1), (NO.CLF, 12), (4, 0)):
        assert L.gx_parse_number(C.byref(fmt(kind, scale)), a.ctypes.data, 3, 0, C.byref(value), C.byref(is_number)) == N.GX_E_ARG


# ---------------------------------------------------------------------------
# the Python side
# ---------------------------------------------------------------------------
def test_python_resolves_names_kinds_and_string_numbers():
    g = three_rules()
    assert g.number_format("alpha", "x") == ("long", 0)
    g.set_number_format("alpha", "x", "iso8601", 3)
    g.set_number_format(2, "z", "decimal", 2)
    g.set_number_format("gamma", 0, "clf")
    assert g.number_format(0, 0) == ("iso8601", 3) and g.number_format("gamma", 2) == ("decimal", 2) and g.number_format(2, 0) == ("clf", 0)
    assert g.number_format("gamma", 1) == ("long", 0)
    for bad in [("delta", "x", "long", 0), (3, 0, "long", 0), ("alpha", "y", "long", 0), ("alpha", 1, "long", 0), ("beta", 0, "long", 0),
                ("gamma", "y", "long", 0),                     # two groups of gamma are called y
                ("alpha", "x", "epoch", 0), ("alpha", "x", 2, 0), ("alpha", "x", "decimal", -1), ("alpha", "x", "decimal", 1.5), ("alpha", "x", "decimal", True)]:
        with pytest.raises(ValueError):
            g.set_number_format(*bad)
    for bad in [("alpha", "x", "long", 1), ("alpha", "x", "decimal", 19), ("alpha", "x", "iso8601", 2), ("alpha", "x", "clf", 10)]:
        with pytest.raises(GorpError) as ei:
            g.set_number_format(*bad)
        assert ei.value.code == N.GX_E_ARG
    assert g.number_format("alpha", "x") == ("iso8601", 3)
    # parse_number: str and bytes
    assert G.parse_number("iso8601", 3, "2026-01-03T04:00:00,25+05:30") == 1767393000250
    assert G.parse_number("iso8601", 3, b"1969-12-31T23:59:59.999Z") == -1
    assert G.parse_number("decimal", 3, "-0.0004") == 0 and G.parse_number("decimal", 0, "12.7") == 12 and G.parse_number("long", 0, "12.7") is None
    assert G.parse_number("clf", 0, "11/Oct/2026:22:14:15 +0200") == 1791749655
    assert G.parse_number("iso8601", 0, "2026-01-03T04:00:00٠") is None and G.parse_number("long", 0, "１") is None and G.parse_number("long", 0, "") is None
    with pytest.raises(ValueError):
        G.parse_number("epoch", 0, "1")
    with pytest.raises(GorpError):
        G.parse_number("iso8601", 4, "1")
    # where_terms: a str as the number of an integer comparison, under the group's format
    w = g.where_terms([("alpha", "x", ">=", "2026-01-03T04:00:00Z"), ("gamma", "z", "<", "1.239"), ("gamma", 0, "<=", "11/Oct/2026:22:14:15 +0200"),
                       ("alpha", "x", ">", 5), ("gamma", 1, ">", 5), ("alpha", "x", "==", "2026")])
    got = [(t.extraction, t.group, t.op, t.negate, t.text_units, t.number) for t in list(w.array)[:w.n]]
    assert got == [(0, 0, N.GX_WHERE_INT_GE, 0, 0, 1767412800000), (2, 2, N.GX_WHERE_INT_LT, 0, 0, 123), (2, 0, N.GX_WHERE_INT_LE, 0, 0, 1791749655),
                   (0, 0, N.GX_WHERE_INT_GT, 0, 0, 5), (2, 1, N.GX_WHERE_INT_GT, 0, 0, 5), (0, 0, N.GX_WHERE_EQ, 0, 4, 0)]   # "==" with a str stays text
    for spec in [("alpha", "x", ">=", "yesterday"), ("alpha", "x", "<", "2026-01-03"), ("gamma", "z", ">", "1e3"), ("gamma", 0, ">", "")]:
        with pytest.raises(GorpError) as ei:
            g.where_terms([spec])
        assert ei.value.code == N.GX_E_ARG and "no number" in ei.value.message
    with pytest.raises(ValueError):
        g.where_terms([("gamma", 1, "<", "5")])                                  # a LONG group takes ints, as before


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def number_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("number") / "number_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "number_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def hexed(units, wide=False):
    return "".join(("%04x" if wide else "%02x") % u for u in units) or "-"


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def check_values(exe, cases):
    """cases: (kind, scale, units, wide)"""
    rows = ["N %s %d %d %s" % ("w" if wide else "b", kind, scale, hexed(units, wide)) for kind, scale, units, wide in cases]
    got = run_cases(exe, rows)
    for (kind, scale, units, wide), g, row in zip(cases, got, rows):
        want = NO.parse(kind, scale, units)
        assert g == ("no" if want is None else str(want)), (row, bytes(u & 0xFF for u in units))


def test_the_case_table_as_bytes_and_as_16_bit_units(number_exe):
    cases = [(kind, scale, tuple(text), wide) for kind, scale, text in NO.table() for wide in (False, True)]
    cases += [(kind, scale, tuple(text), wide) for kind, scale, text, _ in NO.PINNED for wide in (False, True)]
    cases += [(kind, scale, tuple(units), wide) for kind, scale, units, wide in NO.unit_cases()]
    check_values(number_exe, cases)


def test_every_prefix_of_a_number_reads_nothing_behind_its_end(number_exe):
    """Every value cut short at every length, in a buffer of exactly that length: the sanitizer reports a read behind it."""
    whole = [(NO.ISO8601, 9, b"2026-01-03T04:00:00.123456789+05:30"), (NO.ISO8601, 3, b"2026-01-03 04:00:00,5-0530"), (NO.ISO8601, 0, b"2026-01-03t04:00:00z"),
             (NO.CLF, 0, b"11/Oct/2026:22:14:15 +0200x"), (NO.DECIMAL, 18, b"-9.2233720368547758089"), (NO.DECIMAL, 2, b"+123.456"), (NO.LONG, 0, b"-123")]
    cases = [(kind, scale, tuple(text[:n]), wide) for kind, scale, text in whole for n in range(len(text) + 1) for wide in (False, True)]
    check_values(number_exe, cases)


def test_seeded_random_values_of_every_format(number_exe):
    cases = []
    for at, (kind, scale) in enumerate(FORMATS):
        values = NO.random_values(kind, scale, 1500, 100 + at)
        cases += [(kind, scale, tuple(v), False) for v in values] + [(kind, scale, tuple(v), True) for v in values[:300]]
        # ... and each format's values under every other kind: mostly no numbers there
        cases += [(k2, s2, tuple(v), False) for v in values[:60] for k2, s2 in FORMATS if k2 != kind]
    check_values(number_exe, cases)


def test_integer_terms_under_a_format_and_the_formats_a_kind_takes(number_exe):
    values = [(NO.ISO8601, 3, b"1969-12-31T23:59:59.999Z"), (NO.ISO8601, 3, b"1970-01-01T00:00:00Z"), (NO.ISO8601, 3, b"1970-01-01"), (NO.DECIMAL, 3, b"-0.0004"),
              (NO.DECIMAL, 3, b"0.001"), (NO.DECIMAL, 3, b"1e3"), (NO.CLF, 0, b"01/Jan/1970:00:00:01 +0000"), (NO.LONG, 0, b"1"), (NO.LONG, 0, b"1.0")]
    cases = [(kind, scale, op, neg, text, num, wide) for kind, scale, text in values for op in INT_OPS for neg in (0, 1) for num in (-1, 0, 1) for wide in (False, True)]
    rows = ["T %s %d %d %d %d %s %d" % ("w" if wide else "b", kind, scale, op, neg, hexed(text, wide), num) for kind, scale, op, neg, text, num, wide in cases]
    got = run_cases(number_exe, rows)
    for (kind, scale, op, neg, text, num, wide), g, row in zip(cases, got, rows):
        v = NO.parse(kind, scale, text)
        # (where_oracle.holds parses with Long.parseLong: hand it the number's own decimal digits, or what is none)
        want = holds(op, neg, list(b"x" if v is None else b"%d" % v), (), num)
        assert g == ("1" if want else "0"), row
    pairs = [(kind, scale) for kind in range(6) for scale in range(34)]
    got = run_cases(number_exe, ["F %d %d" % p for p in pairs])
    assert got == ["1" if NO.format_ok(*p) else "0" for p in pairs]
