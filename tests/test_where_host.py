"""gx_select_lines_where / gx_text_select_where as far as they go without a GPU: the struct and the symbols, every refusal that needs no
device (and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into terms, and the rule
itself -- gorp_amd/csrc/gx_where.hpp, plain C++ -- built with g++ -fsanitize=address,undefined into tests/cpp/where_test.cpp and run
as a program of its own on cases from here, against a restatement in Python: slices, ==, startswith / endswith / find, and
re.fullmatch(rb"[+-]?[0-9]+") plus a range check."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from where_oracle import INT64_MAX, INT64_MIN, INT_NUMBERS, INT_OPS, INT_TABLE, LITERAL_LENGTHS, TEXT_OPS, holds, near_miss_cases, pair_set, parse_long

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_select_lines_where", "gx_text_select_where"]


# ---------------------------------------------------------------------------
# struct, symbols, refusals
# ---------------------------------------------------------------------------
def three_rules():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),
                           FlattenedExtraction("beta", [["text", "c"]]),
                           FlattenedExtraction("gamma", [["text", "d"], ["extractor", "y", [["pattern", "\\d+"]]], ["extractor", "y", [["pattern", "x*"]]],
                                                         ["extractor", "z", [["pattern", "q?"]]]])], host_only=True)


def opts(**kw):
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_struct_layout_symbols_and_constants():
    T = N.gx_where_term
    assert C.sizeof(T) == 40
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("extraction", 0), ("group", 4), ("op", 8), ("negate", 12), ("text", 16),
                                                                    ("text_units", 24), ("number", 32)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert [N.GX_WHERE_SET, N.GX_WHERE_EQ, N.GX_WHERE_PREFIX, N.GX_WHERE_SUFFIX, N.GX_WHERE_CONTAINS, N.GX_WHERE_INT_EQ, N.GX_WHERE_INT_LT,
            N.GX_WHERE_INT_LE, N.GX_WHERE_INT_GT, N.GX_WHERE_INT_GE] == list(range(10))
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    enum = header[header.index("enum { GX_WHERE_SET = 0"):]
    assert re.findall(r"GX_WHERE_\w+", enum[:enum.index("}")]) == ["GX_WHERE_SET", "GX_WHERE_EQ", "GX_WHERE_PREFIX", "GX_WHERE_SUFFIX", "GX_WHERE_CONTAINS",
                                                                   "GX_WHERE_INT_EQ", "GX_WHERE_INT_LT", "GX_WHERE_INT_LE", "GX_WHERE_INT_GT", "GX_WHERE_INT_GE"]


def term(extraction=0, group=0, op=N.GX_WHERE_SET, negate=0, text=None, text_units=None, number=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.negate, t.number = extraction, group, op, negate, number
    lit = None
    if text is not None:
        lit = np.frombuffer(text, dtype=np.uint8).copy()
        t.text = lit.ctypes.data
        t.text_units = len(lit)
    if text_units is not None:
        t.text_units = text_units
    return t, lit


def test_every_refusal_comes_before_the_look_at_the_device():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    want = np.ones(2 * K + 1, np.uint8)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)

    def both(terms, n_terms=None, caps_ptr=caps.ctypes.data, **kw):
        arr = None
        keep = []
        if terms is not None:
            arr = (N.gx_where_term * max(1, len(terms)))()
            for i, (t, lit) in enumerate(terms):
                arr[i] = t
                keep.append(lit)
        n_terms = len(terms) if n_terms is None else n_terms
        o = opts(**kw)
        k, size = C.c_uint64(0), C.c_uint64(0)
        rc1 = L.gx_select_lines_where(g._h.ptr, data.ctypes.data, offsets.ctypes.data, 3, ids.ctypes.data, caps_ptr, want.ctypes.data, arr, n_terms, None,
                                      None, None, None, None, 0, 0, C.byref(k), C.byref(size), C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_select_where(g._h.ptr, text.ctypes.data, len(text), want.ctypes.data, arr, n_terms, None, 0, C.byref(size), None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        (None, 1),                                                   # terms == NULL with n_terms > 0
        ([term(extraction=-1)], None), ([term(extraction=K)], None),
        ([term(extraction=0, group=1)], None), ([term(extraction=0, group=-1)], None), ([term(extraction=1, group=0)], None),   # beta has no group
        ([term(extraction=2, group=3)], None),
        ([term(op=10)], None), ([term(op=0xFFFFFFFF)], None),
        ([term(op=N.GX_WHERE_EQ, text_units=3)], None),              # a text op with text == NULL and text_units > 0
        ([term(), term(op=N.GX_WHERE_CONTAINS, text_units=1)], None),
    ]
    for terms, n_terms in arg:
        for rc, msg in both(terms, n_terms):
            assert rc == N.GX_E_ARG, (terms, msg)
            assert "no CPU fallback" not in msg
    limit = [[term()] * 65, [term(op=N.GX_WHERE_PREFIX, text=b"x" * 256)], [term(op=N.GX_WHERE_EQ, text=b"x", text_units=256)]]
    for terms in limit:
        for rc, msg in both(terms):
            assert rc == N.GX_E_LIMIT, msg
    # utf8 = 2: offsets in units over a byte buffer
    for rc, msg in both([term()], utf8=2):
        assert rc == N.GX_E_ARG and "utf8" in msg
    for rc, msg in both([], utf8=2):
        assert rc == N.GX_E_ARG and "utf8" in msg
    # dense ids and terms, no caps (the whole-file call makes its own)
    (rc, msg), (rc2, msg2) = both([term()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg
    assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [[], [term()], [term(extraction=2, group=2, op=N.GX_WHERE_INT_GE, number=5)], [term(op=N.GX_WHERE_EQ, text=b"")],
            [term(op=N.GX_WHERE_SUFFIX, text=b"x" * 255)], [term(extraction=k % 3 if k % 3 != 1 else 0) for k in range(64)]]
    for terms in fine:
        for rc, msg in both(terms):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg
    for rc, msg in both([], caps_ptr=None):
        assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.select_lines_where(data, offsets, ids, caps, [("alpha", "x", "==", "b")])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_select_where(bytes(text), [("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.select_lines_where(data, offsets, ids, None, [("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_ARG


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    want = np.ones(7, np.uint8)
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    sizes = (C.c_uint64(0), C.c_uint64(0))

    def select(h, w):
        return L.gx_select_lines_where(h, None, offsets.ctypes.data, 1, ids.ctypes.data, None, w, None, 0, None, None, None, None, None, 0, 0,
                                       C.byref(sizes[0]), C.byref(sizes[1]), C.byref(o))

    for h, w in ((None, want.ctypes.data), (g._h.ptr, None)):
        assert select(h, w) == N.GX_E_ARG and "bad argument" in N.last_error()
        assert L.gx_text_select_where(h, None, 0, w, None, 0, None, 0, C.byref(sizes[0]), None, None, C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# Gorp.where_terms
# ---------------------------------------------------------------------------
def test_where_terms_resolve_names_ops_and_values():
    g = three_rules()
    w = g.where_terms([("alpha", "x", "==", "GET"), (2, "z", "unset"), ("gamma", 1, ">=", 500), ("gamma", 0, "==", 7), (0, 0, "!=", -7),
                       ("alpha", "x", "not contains", b"\xff/"), ("gamma", 2, "set", None), ("alpha", "x", "startswith", ""), ("alpha", 0, "endswith", "é"),
                       ("alpha", "x", "contains", "é"), ("gamma", "z", "<", 1), ("gamma", "z", "<=", 2), ("gamma", "z", ">", INT64_MIN),
                       ("alpha", "x", "!=", "q")])
    got = [(t.extraction, t.group, t.op, t.negate, t.text_units, t.number) for t in list(w.array)[:w.n]]
    assert got == [(0, 0, N.GX_WHERE_EQ, 0, 3, 0), (2, 2, N.GX_WHERE_SET, 1, 0, 0), (2, 1, N.GX_WHERE_INT_GE, 0, 0, 500), (2, 0, N.GX_WHERE_INT_EQ, 0, 0, 7),
                   (0, 0, N.GX_WHERE_INT_EQ, 1, 0, -7), (0, 0, N.GX_WHERE_CONTAINS, 1, 2, 0), (2, 2, N.GX_WHERE_SET, 0, 0, 0),
                   (0, 0, N.GX_WHERE_PREFIX, 0, 0, 0), (0, 0, N.GX_WHERE_SUFFIX, 0, 1, 0), (0, 0, N.GX_WHERE_CONTAINS, 0, 1, 0),
                   (2, 2, N.GX_WHERE_INT_LT, 0, 0, 1), (2, 2, N.GX_WHERE_INT_LE, 0, 0, 2), (2, 2, N.GX_WHERE_INT_GT, 0, 0, INT64_MIN),
                   (0, 0, N.GX_WHERE_EQ, 1, 1, 0)]
    assert C.string_at(w.array[0].text, 3) == b"GET" and C.string_at(w.array[5].text, 2) == b"\xff/"
    assert C.string_at(w.array[8].text, 1) == b"\xe9"                                        # Latin-1 code units
    assert w.array[7].text is None
    assert g.where_terms(w) is w
    u8 = g.where_terms([("alpha", "x", "==", "café")], units="utf-8")
    assert u8.array[0].text_units == 5 and C.string_at(u8.array[0].text, 5) == "café".encode("utf-8")
    u16 = g.where_terms([("alpha", "x", "==", "aЖ\U0001F600")], units="utf-16")
    assert u16.array[0].text_units == 4
    assert np.ctypeslib.as_array(C.cast(u16.array[0].text, C.POINTER(C.c_uint16)), (4,)).tolist() == [0x61, 0x416, 0xD83D, 0xDE00]
    assert g.where_terms([]).n == 0
    # the default want: exactly the extractions that have terms
    assert g._where_want(w, "matched-by-terms").tolist() == [1, 0, 1, 0, 0, 0, 0]
    assert g._where_want(g.where_terms([]), "matched-by-terms").tolist() == [0] * 7
    assert g._where_want(w, ["unmatched", "beta"]).tolist() == [0, 1, 0, 1, 0, 0, 0]
    bad = [("delta", "x", "set"), (3, 0, "set"), (-1, 0, "set"), ("alpha", "y", "set"), ("alpha", 1, "set"), ("beta", 0, "set"),
           ("gamma", "y", "set"),                      # two groups of gamma are called y
           ("alpha", "x", "~=", "a"), ("alpha", "x", "set", "a"), ("alpha", "x", "startswith", 5), ("alpha", "x", "contains", None),
           ("alpha", "x", "<", "5"), ("alpha", "x", ">=", 2 ** 63), ("alpha", "x", "==", "x" * 256), ("alpha", "x", "==", 1.5), ("alpha", "x")]
    for spec in bad:
        with pytest.raises(ValueError):
            g.where_terms([spec])
    with pytest.raises(ValueError):
        g.where_terms([("alpha", "x", "==", "é" * 128)], units="utf-8")    # 256 bytes
    with pytest.raises(ValueError):
        g.where_terms([("alpha", "x", "==", "Ж")])                     # no Latin-1 code unit
    assert g.where_terms([("gamma", 0, "set"), ("gamma", 1, "unset")]).n == 2   # a shared name's groups by index


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def where_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("where") / "where_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "where_test.cpp"), "-o", exe]
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


def check_terms(exe, cases):
    """cases: (op, negate, buffer, begin, end, literal, number, wide); the value is buffer[begin:end] of a line that is the buffer."""
    rows = ["T %s %d %d %s %d %d %s %d" % ("w" if wide else "b", op, neg, hexed(buf, wide), b, e, hexed(lit, wide), num)
            for op, neg, buf, b, e, lit, num, wide in cases]
    got = run_cases(exe, rows)
    for (op, neg, buf, b, e, lit, num, wide), g, row in zip(cases, got, rows):
        value = list(buf[b:e]) if pair_set(b, e, len(buf)) else None
        assert g == ("1" if holds(op, neg, value, lit, num) else "0"), row


def test_every_op_on_every_pair_over_a_small_alphabet(where_exe):
    words = [w for n in range(5) for w in itertools.product(b"-1a", repeat=n)]
    assert len(words) == 121
    cases = [(op, 0, v, 0, len(v), lit, 0, False) for op in TEXT_OPS for v in words for lit in words]
    cases += [(op, neg, v, 0, len(v), (), num, False) for op in INT_OPS + [N.GX_WHERE_SET] for neg in (0, 1) for v in words for num in (-11, -1, 0, 1, 11, 111)]
    cases += [(op, 1, v, 0, len(v), lit, 0, False) for op in TEXT_OPS for v in words[:40] for lit in words[:40]]
    cases += [(op, 0, tuple(0x100 + u for u in v), 0, len(v), tuple(0x100 + u for u in lit), 0, True) for op in TEXT_OPS for v in words[:40] for lit in words[:40]]
    check_terms(where_exe, cases)


def test_literal_lengths_hits_and_near_misses(where_exe):
    lengths = sorted(set(range(0, 41)) | {63, 64, 65, 254, 255, 256, 257, 300})
    cases = near_miss_cases(lengths) + near_miss_cases([0, 1, 4, 5, 16, 17, 64, 255, 300], wide=True)
    assert len(cases) > 5000
    check_terms(where_exe, cases)
    # the value ends where its buffer ends: a literal one unit longer reads nothing behind it (the sanitizer would say so)
    lit = tuple(range(1, 18))
    check_terms(where_exe, [(op, 0, lit[:16], 0, 16, lit, 0, False) for op in TEXT_OPS] + [(op, 0, lit[:16], 0, 16, lit, 0, True) for op in TEXT_OPS])


def test_the_integer_table(where_exe):
    got = run_cases(where_exe, ["I b " + hexed(v) for v in INT_TABLE] + ["I w " + hexed(v, True) for v in INT_TABLE])
    want = [parse_long(v) for v in INT_TABLE] * 2
    assert got == ["no" if v is None else str(v) for v in want]
    assert [v is None for v in want[:16]] == [False] * 6 + [True, False, True] + [True] * 7
    cases = [(op, neg, tuple(v), 0, len(v), (), num, wide) for op in INT_OPS for neg in (0, 1) for v in INT_TABLE for num in INT_NUMBERS for wide in (False, True)]
    # U+FF11 (a digit to Character.digit, not to this rule), and units whose low byte is a digit
    cases += [(op, 0, v, 0, len(v), (), 1, True) for op in INT_OPS for v in ((0xFF11,), (0x31, 0xFF11), (0x131,), (0x31,), (0x2D, 0x31))]
    check_terms(where_exe, cases)


def test_offset_pairs_that_name_no_value(where_exe):
    pairs = [(b, e, n) for n in (0, 1, 5, 200) for b in (-2, -1, 0, 1, 4, 5, 6, 199, 200, 201, 2 ** 31 - 1) for e in (-2, -1, 0, 1, 4, 5, 6, 199, 200, 201, 2 ** 31 - 1)]
    got = run_cases(where_exe, ["P %d %d %d" % p for p in pairs])
    assert got == ["1" if pair_set(*p) else "0" for p in pairs]
    assert pair_set(0, 0, 0) and pair_set(5, 5, 5) and not pair_set(-1, -1, 5) and not pair_set(-1, 3, 5) and not pair_set(3, 2, 5) and not pair_set(0, 6, 5)
    # through a term: pairs that point outside the line are unset -- they fail every test, pass every negated one, and nothing is read
    line = tuple(b"12345")
    cases = [(op, neg, line, b, e, (), 0, False) for op in [N.GX_WHERE_SET] + TEXT_OPS + INT_OPS for neg in (0, 1)
             for b, e in ((-1, -1), (-1, 3), (3, 2), (0, 6), (5, 6), (6, 6), (4, 2 ** 31 - 1), (0, 5), (5, 5), (2, 4))]
    check_terms(where_exe, cases)
