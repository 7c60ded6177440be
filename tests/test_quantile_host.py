"""gx_capture_quantiles / gx_text_capture_quantiles as far as they go without a GPU: the structs and the symbols, every refusal that
needs no device (and "no device is an error, never a CPU path" behind them), the Python side's resolution of quantile spellings, and
the rule itself -- gorp_amd/csrc/gx_quantile.hpp, plain C++ -- built with g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined into tests/cpp/quantile_test.cpp and run as a program of its own on cases from here, against a sort
(tests/quantile_oracle.py)."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from quantile_oracle import ASKS, D32, groups_before_digits, quantiles_of, rank_of, rule_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_capture_quantiles", "gx_text_capture_quantiles"]


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
    Q, O, T = N.gx_quantile, N.gx_quantile_out, N.gx_quantile_totals
    assert C.sizeof(Q) == 8 and [(f, getattr(Q, f).offset) for f, _ in Q._fields_] == [("num", 0), ("den", 4)]
    assert C.sizeof(O) == 32 and [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("value", 0), ("rank", 8), ("below", 16), ("equal", 24)]
    assert dict(O._fields_)["value"] is C.c_int64
    assert C.sizeof(T) == 32 and [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("lines", 0), ("numbers", 8), ("unset", 16), ("not_numbers", 24)]
    assert N.GX_QUANTILE_MAX == 16
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for name in NEW + ["typedef struct gx_quantile ", "typedef struct gx_quantile_out {", "typedef struct gx_quantile_totals {", "#define GX_QUANTILE_MAX 16u"]:
        assert name in header


def part(extraction=0, value_group=0):
    p = N.gx_top_part()
    p.extraction, p.value_group = extraction, value_group
    return p


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


HALF = [(1, 2)]


def test_every_refusal_comes_before_the_look_at_the_device():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    totals = N.gx_quantile_totals()
    out = (N.gx_quantile_out * 32)()

    def both(parts, n_parts=None, terms=(), n_terms=None, qs=HALF, n_qs=None, out_ptr=out, caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals), n=3, off=offsets,
             **kw):
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
        qarr = None
        if qs is not None:
            qarr = (N.gx_quantile * max(1, len(qs)))()
            for i, (num, den) in enumerate(qs):
                qarr[i].num, qarr[i].den = num, den
        n_qs = len(qs) if n_qs is None else n_qs
        o = opts(**kw)
        rc1 = L.gx_capture_quantiles(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, qarr, n_qs, out_ptr,
                                     totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_capture_quantiles(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, qarr, n_qs, out_ptr, totals_ptr, None, None,
                                          C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None),       # totals == NULL
        dict(parts=[part()], qs=None, n_qs=1), dict(parts=[part()], out_ptr=None),    # quantiles == NULL or out == NULL with n_quantiles > 0
        dict(parts=[], qs=None, n_qs=16), dict(parts=[], out_ptr=None, qs=ASKS),
        dict(parts=[part()], qs=[(0, 0)]), dict(parts=[part()], qs=[(1, 2), (1, 0)]), dict(parts=[], qs=[(0, 0)]),   # den == 0
        dict(parts=[part()], qs=[(2, 1)]), dict(parts=[part()], qs=[(1, 1), (D32, D32 - 1)]), dict(parts=[], qs=[(3, 2)]),   # num > den
        dict(parts=None, n_parts=1),                                                  # every refusal of parts that gx_top_lines makes
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(extraction=2, value_group=3)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        # every refusal of a term
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[], terms=[term(extraction=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1), dict(parts=[part()], qs=[], no_sync=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()], qs=ASKS + [(1, 2)]), dict(parts=[], qs=[(1, 2)] * 17), dict(parts=[part()], n_qs=0xFFFFFFFF),   # n_quantiles > GX_QUANTILE_MAX
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
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
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part()], qs=[]), dict(parts=[], qs=[]), dict(parts=[part()], qs=ASKS),
            dict(parts=[part()], qs=None, n_qs=0, out_ptr=None), dict(parts=[part()], qs=[(0, 1), (1, 1), (0, D32), (D32, D32)]),
            dict(parts=[part(2, 2), part()], terms=[term(), term(extraction=2, group=1)]),
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
        g.capture_quantiles(data, offsets, ids, caps, [("alpha", "x")], [0.5])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_capture_quantiles(bytes(text), [("gamma", "z")], ["0.95", (1, 2)], where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.capture_quantiles(data, offsets, ids, None, [("alpha", "x")], [0.5])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(ValueError):
        g.capture_quantiles(data, offsets, ids, caps, [("alpha", "x")], [0.5], utf8="units")
    with pytest.raises(ValueError):
        g.capture_quantiles(data, offsets, ids, caps, [("alpha", "nope")], [0.5])


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_quantile_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_capture_quantiles(h, None, off, 1, id_ptr, None, None, 0, None, 0, None, 0, None, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_capture_quantiles(None, None, 0, None, 0, None, 0, None, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_capture_quantiles(g._h.ptr, None, 5, None, 0, None, 0, None, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# Gorp.quantile_asks
# ---------------------------------------------------------------------------
def test_quantile_spellings_resolve_at_their_decimal_face_value():
    def asks(qs):
        arr, n = Gorp.quantile_asks(qs)
        return [(arr[i].num, arr[i].den) for i in range(n)]
    assert asks([0.99, 0.5, 0.999, 0.0, 1.0, 0.1]) == [(99, 100), (1, 2), (999, 1000), (0, 1), (1, 1), (1, 10)]   # never the float's binary value
    assert asks(["0.95", "1/3", "0", "1", "1e-3"]) == [(19, 20), (1, 3), (0, 1), (1, 1), (1, 1000)]
    assert asks([Fraction(2, 7), Fraction(50, 100), 0, 1, np.float64(0.25)]) == [(2, 7), (1, 2), (0, 1), (1, 1), (1, 4)]
    assert asks([(50, 100), (0, 7), (7, 7), (D32 - 1, D32), [1, 4], (np.int64(3), np.uint32(4))]) == [(50, 100), (0, 7), (7, 7), (D32 - 1, D32), (1, 4), (3, 4)]   # pairs stay as they are
    assert asks([]) == [] and asks([0.5] * 16) == [(1, 2)] * 16 and asks(iter([0.5, 0.5])) == [(1, 2)] * 2
    for bad in (1.5, -0.1, "1.01", "-1/2", Fraction(3, 2), 2, -1, (3, 2), (-1, 2), (1, 0), (0, 0), (1, -2), "x", "", None, True, (1,), (1, 2, 3), (0.5, 1), (True, 1),
                float("nan"), float("inf"), b"0.5", [0.5]):
        with pytest.raises(GorpError) as ei:
            Gorp.quantile_asks([bad])
        assert ei.value.code == N.GX_E_ARG, bad
    for bad in ((1, 2 ** 32), Fraction(1, 2 ** 32 + 1), 0.12345678911, "0.00000000001"):   # a denominator beyond 32 bits
        with pytest.raises(GorpError) as ei:
            Gorp.quantile_asks([bad])
        assert ei.value.code == N.GX_E_LIMIT, bad
    with pytest.raises(GorpError) as ei:
        Gorp.quantile_asks([0.5] * 17)
    assert ei.value.code == N.GX_E_LIMIT
    # refused before the library is called: a handle is not looked at
    g = three_rules()
    with pytest.raises(GorpError) as ei:
        g.capture_quantiles(np.zeros(0, np.uint8), np.zeros(1, np.uint32), np.zeros(0, np.int32), None, [], [1.5])
    assert ei.value.code == N.GX_E_ARG and "[0, 1]" in ei.value.message


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quantile_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quantile") / "quantile_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "quantile_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def test_rank_is_the_nearest_rank_in_integers(quantile_exe):
    rng = random.Random(1)
    cases = [(0, 1, 0), (1, 1, 0), (1, 2, 0), (0, 1, 1), (1, 1, 1), (1, 2, 1), (0, 7, 10), (7, 7, 10), (1, 2, 10), (1, 2, 11), (1, 3, 3), (2, 3, 3), (1, 3, 4),
             (99, 100, 100), (99, 100, 101), (1, 100, 99), (1, 100, 100), (1, 100, 101), (D32, D32, D32 - 1), (D32 - 1, D32, D32 - 1), (1, D32, D32 - 1), (0, D32, D32 - 1)]
    for _ in range(4000):
        den = rng.choice([rng.randint(1, 10), rng.randint(1, 1000), rng.randint(1, D32), D32])
        num = rng.choice([0, den, rng.randint(0, den)])
        numbers = rng.choice([rng.randint(1, 20), rng.randint(1, 10 ** 6), rng.randint(1, D32 - 1), D32 - 1])
        cases.append((num, den, numbers))
    got = [int(x) for x in run_cases(quantile_exe, ["R %d %d %d" % c for c in cases])]
    assert got == [rank_of(*c) for c in cases]
    assert all(1 <= r <= c[2] for r, c in zip(got, cases) if c[2])
    assert [rank_of(0, 5, 9), rank_of(5, 5, 9), rank_of(1, 2, 9), rank_of(1, 2, 10)] == [1, 9, 5, 5]


def pick(hist, remaining):
    """top_pick (tests/test_top_host.py): the bin of the remaining-th largest key, the keys above the bin, what is left to take from it"""
    above = 0
    for b in range(255, -1, -1):
        if above + hist.get(b, 0) >= remaining:
            return b, above, remaining - above
        above += hist.get(b, 0)
    raise AssertionError("remaining exceeds the total")


def test_the_suffix_pick_is_top_pick(quantile_exe):
    rng = random.Random(2)
    hists = [{0: 5}, {255: 5}, {7: 1}, {0: 3, 255: 4}, {0: 1, 1: 1, 254: 1, 255: 1}, {10: 2, 20: 3, 30: 4}, {b: 1 for b in range(256)},
             {b: b + 1 for b in range(256)}, {128: 2 ** 32 - 2}, {0: 2 ** 31, 255: 2 ** 31 - 1}]
    for _ in range(300):
        hists.append({rng.randrange(256): rng.choice([1, 2, rng.randrange(1, 1000)]) for _ in range(rng.choice([1, 2, 5, 40, 256]))})
    cases = []
    for h in hists:
        total, run = sum(h.values()), 0
        ranks = {1, total, rng.randint(1, total)}
        for b in sorted(h, reverse=True):
            run += h[b]
            ranks |= {run, run + 1, run - 1}                      # on a bin's boundary, just behind it, just before it
        cases += [(h, r) for r in sorted(ranks) if 1 <= r <= total]
    assert len(cases) > 5000
    got = run_cases(quantile_exe, ["P %d %d %s" % (r, len(h), " ".join("%d %d" % bc for bc in h.items())) for h, r in cases])   # (status 3: not top_pick's)
    assert [tuple(int(x) for x in g.split()) for g in got] == [pick(h, r) for h, r in cases]


def check_select(exe, cases):
    rows = ["Q %d %s %d %s" % (len(asks), " ".join("%d %d" % a for a in asks), len(vs), " ".join(map(str, vs))) for vs, asks in cases]
    for (vs, asks), g in zip(cases, run_cases(exe, rows)):
        nums = [int(x) for x in g.split()]
        got = [dict(zip(("value", "rank", "below", "equal"), nums[4 * q:4 * q + 4])) for q in range(len(asks))]
        groups = nums[4 * len(asks):]
        want = quantiles_of(vs, asks)
        for w in want:
            if w["value"] is None:
                w["value"] = 0                                    # (the rule's row is all zeros; None is the Python side's)
        assert got == want, (vs[:20], asks, got, want)
        assert all(w["below"] < w["rank"] <= w["below"] + w["equal"] for w in want if vs)
        assert len(groups) == 8 and groups[0] == (1 if asks else 0) and max(groups) <= 16
        if vs and asks:
            assert groups == groups_before_digits([w["value"] for w in want]), (vs[:20], asks, groups)


def test_the_host_select_equals_a_sort(quantile_exe):
    cases = rule_cases()
    assert any(len(vs) == 1 for vs, _ in cases) and any(len(vs) == 2 for vs, _ in cases) and any(len(vs) == 255 for vs, _ in cases)
    check_select(quantile_exe, cases)
    # the parting population: the 16 quantiles' prefixes part at every one of the eight digits
    parting = [c for c in cases if len(c[0]) == 16 and len(c[1]) == 16 and c[1][0] == (1, 16)][0]
    got = quantiles_of(*parting)
    assert groups_before_digits([w["value"] for w in got]) == [1, 2, 3, 4, 5, 6, 7, 8] and len({w["value"] for w in got}) == 16
    # random populations of few values (ties everywhere) and of many, with random quantiles
    rng = random.Random(3)
    more = []
    for _ in range(400):
        count = rng.choice([1, 2, 3, 10, 64, 300])
        span = rng.choice([3, 300, 2 ** 20, 2 ** 62])
        vs = [rng.randint(-span, span) for _ in range(count)]
        asks = []
        for _ in range(rng.choice([1, 3, 16])):
            den = rng.choice([1, 2, 100, count, rng.randint(1, D32), D32])
            asks.append((rng.choice([0, den, rng.randint(0, den)]), den))
        more.append((vs, asks))
    check_select(quantile_exe, more)
