"""gx_capture_stats / gx_text_capture_stats as far as they go without a GPU: the structs and the symbols, every refusal that needs no
device (and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into measures, and the rule
itself -- gorp_amd/csrc/gx_stats.hpp, plain C++ -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into
tests/cpp/stats_test.cpp and run as a program of its own on cases from here, against Python's integers (tests/stats_oracle.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, Measures
from stats_oracle import SUM_SEQUENCES, bucket, split128, summarise
from where_oracle import INT64_MAX, INT64_MIN, INT_TABLE, parse_long

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_capture_stats", "gx_text_capture_stats"]


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
    M, S = N.gx_measure, N.gx_measure_stats
    assert C.sizeof(M) == 24
    assert [(f, getattr(M, f).offset) for f, _ in M._fields_] == [("extraction", 0), ("group", 4), ("edges", 8), ("n_edges", 16)]
    assert C.sizeof(S) == 64
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("lines", 0), ("numbers", 8), ("unset", 16), ("not_numbers", 24), ("min", 32), ("max", 40),
                                                                    ("sum_lo", 48), ("sum_hi", 56)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for name in NEW + ["typedef struct gx_measure {", "typedef struct gx_measure_stats {"]:
        assert name in header


def measure(extraction=0, group=0, edges=None, n_edges=None):
    m = N.gx_measure()
    m.extraction, m.group = extraction, group
    arr = None
    if edges is not None:
        arr = np.array(edges, dtype=np.int64)
        m.edges = arr.ctypes.data if arr.size else None
        m.n_edges = arr.size
    if n_edges is not None:
        m.n_edges = n_edges
    return m, arr


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
    stats = (N.gx_measure_stats * 80)()
    hist = np.zeros(2048, np.uint64)

    def both(measures, n_measures=None, terms=(), n_terms=None, caps_ptr=caps.ctypes.data, stats_ptr=stats, **kw):
        arr, keep = None, []
        if measures is not None:
            arr = (N.gx_measure * max(1, len(measures)))()
            for i, (m, edges) in enumerate(measures):
                arr[i] = m
                keep.append(edges)
        n_measures = len(measures) if n_measures is None else n_measures
        tarr = None
        if terms is not None:
            tarr = (N.gx_where_term * max(1, len(terms)))()
            for i, t in enumerate(terms):
                tarr[i] = t
        n_terms = len(terms) if n_terms is None else n_terms
        o = opts(**kw)
        rc1 = L.gx_capture_stats(g._h.ptr, data.ctypes.data, offsets.ctypes.data, 3, ids.ctypes.data, caps_ptr, arr, n_measures, tarr, n_terms, stats_ptr,
                                 hist.ctypes.data, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_capture_stats(g._h.ptr, text.ctypes.data, len(text), arr, n_measures, tarr, n_terms, stats_ptr, hist.ctypes.data, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        dict(measures=None, n_measures=1),                                    # measures == NULL with n_measures > 0
        dict(measures=[measure()], stats_ptr=None),                           # stats == NULL
        dict(measures=[measure(extraction=-1)]), dict(measures=[measure(extraction=K)]),
        dict(measures=[measure(extraction=0, group=1)]), dict(measures=[measure(group=-1)]), dict(measures=[measure(extraction=1, group=0)]),   # beta has no group
        dict(measures=[measure(extraction=2, group=3)]),
        dict(measures=[measure(n_edges=1)]),                                  # edges == NULL with n_edges > 0
        dict(measures=[measure(edges=[1, 1])]), dict(measures=[measure(edges=[2, 1])]), dict(measures=[measure(edges=[0, 5, 5, 9])]),
        dict(measures=[measure(), measure(extraction=2, group=2, edges=[INT64_MAX, INT64_MIN])]),
        # every refusal of a term
        dict(measures=[measure()], terms=None, n_terms=1), dict(measures=[measure()], terms=[term(extraction=K)]), dict(measures=[measure()], terms=[term(group=1)]),
        dict(measures=[measure()], terms=[term(op=10)]), dict(measures=[measure()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(measures=[], terms=[term(extraction=1)]),
        dict(measures=[measure()], utf8=2), dict(measures=[], utf8=2),
        dict(measures=[measure()], no_sync=1, device_pointers=1), dict(measures=[], no_sync=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(measures=[measure()] * 65),
        dict(measures=[measure(edges=list(range(65)))]),
        dict(measures=[measure()], terms=[term()] * 65),
        dict(measures=[measure(edges=list(range(17)))] + [measure(edges=list(range(16)))] * 63),         # 1 025 edges
        dict(measures=[measure(edges=list(range(64)))] * 16 + [measure(edges=[3])]),
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    # measures or terms on dense ids without caps (the whole-file call makes its own)
    for kw in (dict(measures=[measure()]), dict(measures=[], terms=[term()])):
        (rc, msg), (rc2, msg2) = both(caps_ptr=None, **kw)
        assert rc == N.GX_E_ARG and "caps" in msg
        assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(measures=[]), dict(measures=[], stats_ptr=None), dict(measures=[measure()]), dict(measures=[measure(edges=[])]),
            dict(measures=[measure(edges=[INT64_MIN, 0, INT64_MAX])]), dict(measures=[measure(edges=list(range(64)))]),
            dict(measures=[measure(edges=list(range(16)))] * 64),                                          # 1 024 edges
            dict(measures=[measure(extraction=2, group=2), measure(), measure(extraction=2, group=0, edges=[5])], terms=[term(), term(extraction=2, group=1)]),
            dict(measures=[measure()] * 64, terms=[term()] * 64), dict(measures=[measure()], utf8=1), dict(measures=[measure()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(measures=[measure()], utf16=1)
    assert rc == N.GX_E_DEVICE
    (rc, msg), _ = both(measures=[measure()], compact_results=3)
    assert rc == N.GX_E_ARG
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.capture_stats(data, offsets, ids, caps, [("alpha", "x", [1, 2])])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_capture_stats(bytes(text), [("gamma", "z")], where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.capture_stats(data, offsets, ids, None, [("alpha", "x")])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(ValueError):
        g.capture_stats(data, offsets, ids, caps, [("alpha", "x")], utf8="units")


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_capture_stats(h, None, off, 1, id_ptr, None, None, 0, None, 0, None, None, C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_capture_stats(None, None, 0, None, 0, None, 0, None, None, None, None, C.byref(o)) == N.GX_E_ARG and "bad argument" in N.last_error()
    assert L.gx_text_capture_stats(g._h.ptr, None, 5, None, 0, None, 0, None, None, None, None, C.byref(o)) == N.GX_E_ARG and "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# Gorp.measures
# ---------------------------------------------------------------------------
def test_measures_resolve_names_groups_and_edges():
    g = three_rules()
    m = g.measures([("alpha", "x", [10, 100, 500, 1000]), (2, "z"), ("gamma", 1, None), ("gamma", 0, [INT64_MIN, INT64_MAX]), (0, 0, []),
                    ("alpha", "x", np.array([-5, 5]))])
    assert isinstance(m, Measures) and m.n == 6 and m.n_bins == 5 + 1 + 1 + 3 + 1 + 3
    assert [(t.extraction, t.group, t.n_edges) for t in list(m.array)[:m.n]] == [(0, 0, 4), (2, 2, 0), (2, 1, 0), (2, 0, 2), (0, 0, 0), (0, 0, 2)]
    assert np.ctypeslib.as_array(C.cast(m.array[0].edges, C.POINTER(C.c_int64)), (4,)).tolist() == [10, 100, 500, 1000]
    assert np.ctypeslib.as_array(C.cast(m.array[3].edges, C.POINTER(C.c_int64)), (2,)).tolist() == [INT64_MIN, INT64_MAX]
    assert m.array[1].edges is None and m.array[4].edges is None
    assert [e.tolist() for e in m.edges] == [[10, 100, 500, 1000], [], [], [INT64_MIN, INT64_MAX], [], [-5, 5]]      # (kept alive)
    assert g.measures(m) is m
    assert g.measures([]).n == 0 and g.measures([]).n_bins == 0
    bad = [("delta", "x"), (3, 0), (-1, 0), ("alpha", "y"), ("alpha", 1), ("beta", 0),
           ("gamma", "y"),                      # two groups of gamma are called y
           ("alpha", "x", [1, 1]), ("alpha", "x", [2, 1]), ("alpha", "x", [1.5]), ("alpha", "x", ["1"]), ("alpha", "x", [2 ** 63]), ("alpha", "x", [True]),
           ("alpha", "x", list(range(65))), ("alpha",), ("alpha", "x", [1], 2)]
    for spec in bad:
        with pytest.raises(ValueError):
            g.measures([spec])
    with pytest.raises(ValueError):
        g.measures([("alpha", "x")] * 65)
    with pytest.raises(ValueError):
        g.measures([("alpha", "x", list(range(17)))] + [("alpha", "x", list(range(16)))] * 63)
    assert g.measures([("alpha", "x", list(range(16)))] * 64).n_bins == 64 * 17
    assert g.measures([("gamma", 0), ("gamma", 1)]).n == 2   # a shared name's groups by index


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats") / "stats_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "stats_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


EDGE_SETS = [[], [0], [INT64_MIN], [INT64_MAX], [INT64_MIN, INT64_MAX], [INT64_MIN, -1, 0, 1, INT64_MAX], [10, 100, 500, 1000], list(range(-320, 320, 10)),
             [INT64_MIN + 3 * j for j in range(32)] + [INT64_MAX - 3 * j for j in range(31, -1, -1)], [7 * j * j * j for j in range(-31, 32)]]


def probes(edges):
    out = {INT64_MIN, -1, 0, 1, INT64_MAX}
    for e in edges:
        out |= {v for v in (e - 1, e, e + 1) if INT64_MIN <= v <= INT64_MAX}
    return sorted(out)


def test_bucket_on_below_and_above_every_edge(stats_exe):
    assert [len(e) for e in EDGE_SETS[:2]] == [0, 1] and sorted(len(e) for e in EDGE_SETS)[-2:] == [64, 64]
    cases = [(edges, v) for edges in EDGE_SETS for v in probes(edges)]
    got = run_cases(stats_exe, ["B %d %s %d" % (len(e), " ".join(map(str, e)), v) for e, v in cases])
    assert [int(x) for x in got] == [bucket(e, v) for e, v in cases]
    assert bucket([10, 100], 9) == 0 and bucket([10, 100], 10) == 1 and bucket([10, 100], 100) == 2 and bucket([], 5) == 0


def expand(runs):
    return [v for count, v in runs for _ in range(count)]


def test_sums_that_leave_int64_in_both_directions(stats_exe):
    sequences = dict(SUM_SEQUENCES)
    sequences["classes"] = [(3, "u"), (5, 17), (2, "x"), (1, -17), (4, "u")]
    sequences["empty"] = []
    sequences["one"] = [(1, INT64_MIN)]
    rows, want = [], []
    for name, runs in sequences.items():
        for chunk in (1, 64, 256, 1000, 10 ** 9):          # (how many lines an accumulator takes before it is merged)
            rows.append("A %d %d %s" % (chunk, len(runs), " ".join("%d %s" % r for r in runs)))
            values = [None if v == "u" else b"x" if v == "x" else str(v).encode() for v in expand(runs)]
            want.append(summarise(values, []))
    got = run_cases(stats_exe, rows)
    for row, g, w in zip(rows, got, want):
        lines, numbers, unset, nan, mn, mx, lo, hi, sum_hi, sum_lo = (int(x) for x in g.split())
        assert (lines, numbers, unset, nan) == (w["lines"], w["numbers"], w["unset"], w["not_numbers"]), row
        assert (mn, mx) == ((w["min"], w["max"]) if numbers else (INT64_MAX, INT64_MIN)), row
        assert hi * 2 ** 32 + lo == w["sum"] and (sum_hi, sum_lo) == split128(w["sum"]), row
    up, down, mixed = (sum(expand(SUM_SEQUENCES[k])) for k in ("up", "down", "mixed"))
    assert up > INT64_MAX and down < INT64_MIN
    mixed_hi = sum(v >> 32 for v in expand(SUM_SEQUENCES["mixed"]))
    assert mixed_hi < 0 and sum(v & 0xFFFFFFFF for v in expand(SUM_SEQUENCES["mixed"])) > 2 ** 32      # hi is negative while lo carries


def test_the_128_bit_combine(stats_exe):
    rng = np.random.default_rng(5)
    pairs = [(lo, hi) for lo in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1) for hi in (0, 1, -1, 2 ** 31, -2 ** 31, 2 ** 32, -2 ** 32, 2 ** 63 - 1, -2 ** 63)]
    pairs += [(int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(-2 ** 63, 2 ** 63 - 1))) for _ in range(200)]
    got = run_cases(stats_exe, ["C %d %d" % p for p in pairs])
    assert [tuple(int(x) for x in g.split()) for g in got] == [split128(hi * 2 ** 32 + lo) for lo, hi in pairs]


def test_one_value_is_classed_then_added(stats_exe):
    hexed = lambda units, wide: "".join(("%04x" if wide else "%02x") % u for u in units) or "-"
    edges = [10, 100, 500, 1000]
    cases = [(tuple(v), wide, 1) for v in INT_TABLE for wide in (False, True)] + [(tuple(b"12"), False, 0), ((), True, 0)]
    cases += [((0xFF11,), True, 1), ((0x31, 0xFF11), True, 1), ((0x131,), True, 1), ((0x31, 0x30, 0x30), True, 1)]   # U+FF11 is no digit here
    got = run_cases(stats_exe, ["S %s %s %d %d %s" % ("w" if wide else "b", hexed(v, wide), s, len(edges), " ".join(map(str, edges))) for v, wide, s in cases])
    for (v, wide, s), g in zip(cases, got):
        number = parse_long(list(v)) if s else None
        if not s:
            want = "unset 0 %d %d" % (INT64_MAX, INT64_MIN)
        elif number is None:
            want = "nan 0 %d %d" % (INT64_MAX, INT64_MIN)
        else:
            want = "%d 1 %d %d" % (bucket(edges, number), number, number)
        assert g == want, (v, wide, s)
    assert got[-1].startswith("2 1 100") and got[-4].startswith("nan")
