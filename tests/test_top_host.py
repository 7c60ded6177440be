"""gx_top_lines / gx_text_top_lines as far as they go without a GPU: the structs and the symbols, every refusal that needs no device
(and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into parts, and the rule itself --
gorp_amd/csrc/gx_top.hpp, plain C++ -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into
tests/cpp/top_test.cpp and run as a program of its own on cases from here, against Python's sorted() (tests/top_oracle.py)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, TopParts
from top_oracle import decode_parts, rank
from where_oracle import INT64_MAX, INT64_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_top_lines", "gx_text_top_lines"]


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


# ---------------------------------------------------------------------------
# structs, symbols, refusals
# ---------------------------------------------------------------------------
def test_struct_layouts_and_symbols():
    P, T = N.gx_top_part, N.gx_top_totals
    assert C.sizeof(P) == 8
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("extraction", 0), ("value_group", 4)]
    assert C.sizeof(T) == 64
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("lines", 0), ("numbers", 8), ("unset", 16), ("not_numbers", 24), ("n_top", 32),
                                                                    ("units_top", 40), ("last_value", 48), ("ties_left", 56)]
    assert dict(T._fields_)["last_value"] is C.c_int64
    assert N.GX_TOP_SMALLEST == 1 and N.GX_TOP_MAX_LINES >= 4096
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for name in NEW + ["typedef struct gx_top_part {", "typedef struct gx_top_totals {", "#define GX_TOP_SMALLEST 1u", "#define GX_TOP_MAX_LINES %du" % N.GX_TOP_MAX_LINES]:
        assert name in header


def part(extraction=0, value_group=0):
    p = N.gx_top_part()
    p.extraction, p.value_group = extraction, value_group
    return p


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


def test_every_refusal_comes_before_the_look_at_the_device():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    totals = N.gx_top_totals()

    def both(parts, n_parts=None, terms=(), n_terms=None, n_wanted=2, flags=0, caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals), n=3, off=offsets, **kw):
        arr = None
        if parts is not None:
            arr = (N.gx_top_part * max(1, len(parts)))()
            for i, p in enumerate(parts):
                arr[i] = p
        n_parts = len(parts) if n_parts is None else n_parts
        tarr = None
        if terms is not None:
            tarr = (N.gx_where_term * max(1, len(terms)))()
            for i, t in enumerate(terms):
                tarr[i] = t
        n_terms = len(terms) if n_terms is None else n_terms
        o = opts(**kw)
        rc1 = L.gx_top_lines(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, n_wanted, flags, None, None,
                             None, None, None, None, 0, 0, totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_top_lines(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, n_wanted, flags, None, None, None, 0, None, totals_ptr,
                                  None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None),       # totals == NULL
        dict(parts=None, n_parts=1),                                                  # parts == NULL with n_parts > 0
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),          # a part out of range
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(extraction=2, value_group=3)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        dict(parts=[part()], flags=2), dict(parts=[], flags=0x80000000), dict(parts=[part()], flags=3),   # unknown flag bits
        # every refusal of a term
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[], terms=[term(extraction=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
        dict(parts=[part()], n_wanted=N.GX_TOP_MAX_LINES + 1), dict(parts=[], n_wanted=0xFFFFFFFF),
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    # n of 2^32 - 1 and more; a line of 2^32 units or more, and offsets that go backwards (host offsets: read without a device)
    (rc, msg), _ = both(parts=[part()], n=0xFFFFFFFF)
    assert rc == N.GX_E_LIMIT and "2^32 - 1" in msg
    for off in (np.array([0, 2, 5, 5 + 2 ** 32], np.uint64), np.array([0, 2, 1, 7], np.uint64)):
        (rc, msg), _ = both(parts=[part()], off=off, offsets64=1)
        assert rc == N.GX_E_LIMIT and "4 G code units" in msg
    # parts or terms on dense ids without caps (the whole-file call makes its own)
    for kw in (dict(parts=[part()]), dict(parts=[], terms=[term()])):
        (rc, msg), (rc2, msg2) = both(caps_ptr=None, **kw)
        assert rc == N.GX_E_ARG and "caps" in msg
        assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part()], n_wanted=0), dict(parts=[], n_wanted=0), dict(parts=[part()], n_wanted=N.GX_TOP_MAX_LINES),
            dict(parts=[part()], flags=N.GX_TOP_SMALLEST), dict(parts=[part(2, 2), part()], terms=[term(), term(extraction=2, group=1)]),
            dict(parts=[part(2, 0), part()], terms=[term()] * 64), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2),
            dict(parts=[part()], n=0xFFFFFFFE, device_pointers=1)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    (rc, msg), _ = both(parts=[part()], compact_results=3)
    assert rc == N.GX_E_ARG
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.top_lines(data, offsets, ids, caps, [("alpha", "x")], 3)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_top_lines(bytes(text), [("gamma", "z")], 1, largest=False, where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.top_lines(data, offsets, ids, None, [("alpha", "x")], 3)
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(GorpError) as ei:
        g.top_lines(data, offsets, ids, caps, [("alpha", "x")], N.GX_TOP_MAX_LINES + 1)
    assert ei.value.code == N.GX_E_LIMIT
    with pytest.raises(ValueError):
        g.top_lines(data, offsets, ids, caps, [("alpha", "x")], 3, utf8="units")


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_top_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_top_lines(h, None, off, 1, id_ptr, None, None, 0, None, 0, 1, 0, None, None, None, None, None, None, 0, 0, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_top_lines(None, None, 0, None, 0, None, 0, 1, 0, None, None, None, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_top_lines(g._h.ptr, None, 5, None, 0, None, 0, 1, 0, None, None, None, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# Gorp.top_parts
# ---------------------------------------------------------------------------
def test_top_parts_resolve_names_and_groups():
    g = three_rules()
    p = g.top_parts([("alpha", "x"), (2, "z")])
    assert isinstance(p, TopParts) and p.n == 2
    assert decode_parts(p) == [(0, 0), (2, 2)]
    assert g.top_parts(p) is p
    assert g.top_parts([]).n == 0
    assert decode_parts(g.top_parts([("gamma", 1)])) == [(2, 1)]          # a shared name's group by index
    assert decode_parts(g.top_parts([(np.int64(2), np.int32(0)), (0, 0)])) == [(2, 0), (0, 0)]
    bad = [("delta", "x"), (3, 0), (-1, 0), ("alpha", "y"), ("alpha", 1), ("beta", 0),
           ("gamma", "y"),                      # two groups of gamma are called y
           ("alpha",), ("alpha", "x", "x"), (True, 0)]
    for spec in bad:
        with pytest.raises(ValueError):
            g.top_parts([spec])
    with pytest.raises(ValueError):
        g.top_parts([("alpha", "x"), (0, 0)])   # two parts for one extraction
    with pytest.raises(ValueError):
        g.top_parts([("alpha", "x")] * 65)


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def top_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top") / "top_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "top_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def key_table():
    table = {0, 1, -1, INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1}
    for d in range(8):
        for sign in (1, -1):
            for delta in (-1, 0, 1):
                table.add(sign * 2 ** (8 * d) + delta)
    return sorted(v for v in table if INT64_MIN <= v <= INT64_MAX)


def test_key_is_strictly_monotone_in_both_directions(top_exe):
    table = key_table()
    assert len(table) > 40 and table[0] == INT64_MIN and table[-1] == INT64_MAX
    for smallest in (0, 1):
        got = [tuple(int(x) for x in g.split()) for g in run_cases(top_exe, ["K %d %d" % (smallest, v) for v in table])]
        keys = [k for k, _ in got]
        assert [back for _, back in got] == table                                   # the map goes back
        assert all(0 <= k < 2 ** 64 for k in keys)
        if smallest:
            assert all(a > b for a, b in zip(keys, keys[1:]))                       # value ascending = key descending
            assert keys == [(2 ** 64 - 1) - ((v + 2 ** 63) % 2 ** 64) for v in table]   # the complement, never a negation
        else:
            assert all(a < b for a, b in zip(keys, keys[1:]))
            assert keys == [v + 2 ** 63 for v in table]                             # the sign bit flipped
    keys = [0, 1, 0xFF, 0x100, 0x0123456789ABCDEF, 2 ** 64 - 1, 2 ** 63]
    got = run_cases(top_exe, ["D %d %d" % (k, d) for k in keys for d in range(8)])
    assert [int(x) for x in got] == [(k >> (8 * d)) & 0xFF for k in keys for d in range(8)]


def pick(hist, remaining):
    """the bin of the remaining-th largest key, the keys above the bin, and what is left to take from it"""
    above = 0
    for b in range(255, -1, -1):
        if above + hist.get(b, 0) >= remaining:
            return b, above, remaining - above
        above += hist.get(b, 0)
    raise AssertionError("remaining exceeds the total")


def test_pick_finds_the_bin_of_the_rank(top_exe):
    hists = [{0: 5}, {255: 5}, {7: 1}, {0: 3, 255: 4}, {0: 1, 1: 1, 254: 1, 255: 1}, {10: 2, 20: 3, 30: 4}, {b: 1 for b in range(256)},
             {b: b + 1 for b in range(256)}, {128: 2 ** 32 - 2}, {0: 2 ** 31, 255: 2 ** 31 - 1}]
    cases = []
    for h in hists:
        total, run = sum(h.values()), 0
        ranks = {1, total}                                        # in the first bin from the top; remaining equal to the total: the last bin
        for b in sorted(h, reverse=True):
            run += h[b]
            ranks |= {run, run + 1, run - 1}                      # on a bin's boundary, just behind it, just before it
        cases += [(h, r) for r in sorted(ranks) if 1 <= r <= total]
    got = run_cases(top_exe, ["P %d %d %s" % (r, len(h), " ".join("%d %d" % bc for bc in h.items())) for h, r in cases])
    assert [tuple(int(x) for x in g.split()) for g in got] == [pick(h, r) for h, r in cases]
    assert pick({10: 2, 20: 3, 30: 4}, 4) == (30, 0, 4) and pick({10: 2, 20: 3, 30: 4}, 5) == (20, 4, 1) and pick({10: 2, 20: 3, 30: 4}, 9) == (10, 7, 2)
    assert pick({7: 1}, 1) == (7, 0, 1)                           # all mass in one bin


ALPHABET = [INT64_MIN, -256, -1, 0, 1, 255, 2 ** 32, INT64_MAX]


def test_the_host_select_equals_sorted_on_every_small_multiset(top_exe):
    cases = []
    for count in range(6):
        for values in itertools.product(ALPHABET, repeat=count) if count <= 3 else itertools.combinations_with_replacement(ALPHABET, count):
            orders = [values] if count <= 3 else [values, values[::-1], values[1::2] + values[::2]]
            for vs in orders:
                for n in sorted({0, 1, 2, count - 1, count, count + 1} - {-1}):
                    for smallest in (0, 1):
                        cases.append((smallest, n, list(vs)))
    assert len(cases) > 20000
    got = run_cases(top_exe, ["S %d %d %d %s" % (s, n, len(vs), " ".join(map(str, vs))) for s, n, vs in cases])
    for (smallest, n, vs), g in zip(cases, got):
        n_top, threshold, above, taken, *chosen = (int(x) for x in g.split())
        top = rank([(v, i) for i, v in enumerate(vs)], n, largest=not smallest)
        assert n_top == len(top) == min(n, len(vs)), (smallest, n, vs)
        assert chosen == sorted(i for _, i in top), (smallest, n, vs, g)              # the chosen ones, in line order
        if top:
            last = top[-1][0]
            assert threshold == last and taken == sum(1 for v, _ in top if v == last) and above == n_top - taken, (smallest, n, vs, g)
        else:
            assert (threshold, above, taken) == (0, 0, 0)
