"""gx_group_series / gx_text_group_series as far as they go without a GPU: the structs, the symbols and the header's text, every refusal
that needs no device, in order (and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into
parts, and the rule itself -- cell_word, sort_word, the digit count and find-or-insert over both tables of gorp_amd/csrc/gx_series.hpp,
plain C++, with the host policy -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into
tests/cpp/series_test.cpp and run as a program of its own, against the Python forms (tests/series_oracle.py).  The numpy restatement
that the large GPU case is compared with is compared with the oracle here, on small draws of the same generator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, GroupParts
from bucket_oracle import INT64_MIN, M64, bucket_hash, word_of
from series_oracle import (SERIES_FIELDS, cell_bslot, cell_kslot, cell_word, decode_parts, digits_batch, draw, group_series, np_series, series_digits,
                           sort_word)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_series", "gx_text_group_series"]


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
# structs, symbols, the header's text
# ---------------------------------------------------------------------------
def test_struct_layouts_symbols_and_header_text():
    O, T = N.gx_series_out, N.gx_series_totals
    assert C.sizeof(O) == 80
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("bucket_number", 0), ("cell_key", 8), ("cell_bucket", 16), ("cell_first_line", 24), ("cell_lines", 32),
                                                                    ("cell_stats", 40), ("key_cell_begin", 48), ("line_cell", 56), ("max_cells", 64), ("max_buckets", 72)]
    g = C.sizeof(N.gx_group_totals)
    assert C.sizeof(T) == g + 72
    assert [(f, getattr(T, f).offset - g) for f, _ in T._fields_[1:]] == [("n_cells", 0), ("n_buckets", 8), ("celled", 16), ("number_unset", 24), ("not_numbers", 32),
                                                                           ("out_of_range", 40), ("cells_exact", 48), ("first_bucket", 56), ("last_bucket", 64)]
    assert T.group.offset == 0
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["typedef struct gx_series_out {", "typedef struct gx_series_totals {",
                       "perVerb.computeIfAbsent(r.asMap().get(\"verb\"), v -> new TreeMap<Long, Stats>())", "GROUP BY verb, floor((ts - origin) / width)",
                       "keyed == celled + number_unset + not_numbers +\n * out_of_range", "HOW THE BATCH IS READ: exactly as gx_group_lines reads it",
                       "GX_BUCKET_ALL_DIGITS (it applies to both sorts)", "With series == NULL the call IS gx_group_lines", "cells_exact = 0 and n_cells\n * = slots + 1",
                       "The number of lines is always a sufficient\n * max_cells", "EMPTY INPUTS: n == 0 and n_parts == 0 are legal", "ONE host wait before any output",
                       "NOT IN SCOPE: empty cells filled in, calendar widths, quantiles per cell, ranking cells, lines per bucket across keys"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_series.hpp")).read()
    for text in ["Not in scope: empty cells filled in, calendar widths", "more than one text key (compose with gx_group_pairs later)",
                 "cell_word(uint32_t kslot, uint32_t bslot)", "sort_word(uint64_t key_number, uint64_t bucket_rank, uint64_t n_buckets)", "struct SeriesHead",
                 "struct SeriesDev", "complete the moment it\n// is visible"]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule and "__int128" not in rule


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    return N.gx_group_part(extraction, key_group, value_group, reserved)


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


def test_every_refusal_comes_before_the_look_at_the_device_in_order():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    buf = np.zeros(64, np.uint64)

    def both(parts, numbers=(), n_parts=None, numbers_null=False, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, series=True, outputs=(), max_cells=8,
             max_keys=8, n=3, origin=0, width=1, **kw):
        arr = None if parts is None else (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        numbers = list(numbers) + [0] * (n_parts - len(numbers))
        narr = None if numbers_null else (C.c_int32 * max(1, len(numbers)))(*numbers)
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        ko = N.gx_group_out()
        ko.max_keys = max_keys
        so = N.gx_series_out()
        so.max_cells, so.max_buckets = max_cells, 8
        for name in outputs:
            setattr(so, name, buf.ctypes.data)
        tot = N.gx_series_totals()
        tp = C.byref(tot) if totals else None
        sp = C.byref(so) if series else None
        rc1 = L.gx_group_series(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, narr, origin, width, tarr, len(terms), flags,
                                C.byref(ko), sp, tp, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_series(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, narr, origin, width, tarr, len(terms), flags, C.byref(ko), sp, tp, None, None,
                                     C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    every_output = ("bucket_number", "cell_key", "cell_bucket", "cell_first_line", "cell_lines", "key_cell_begin", "line_cell")
    arg = [
        # what gx_group_series adds
        dict(parts=[part()], numbers_null=True), dict(parts=[part()], numbers=[1]), dict(parts=[part()], numbers=[-2]), dict(parts=[part(extraction=2)], numbers=[3]),
        dict(parts=[part()], width=0), dict(parts=[part()], width=-1), dict(parts=[], width=0), dict(parts=[part()], width=INT64_MIN),
        dict(parts=[part()], outputs=("cell_stats",)), dict(parts=[], outputs=("cell_stats",)),
        dict(parts=[part()], numbers=[-1], outputs=("cell_key",)), dict(parts=[part(), part(extraction=2)], numbers=[-1, -1], outputs=("line_cell",)),
        dict(parts=[part()], numbers=[-1], outputs=("bucket_number",)), dict(parts=[part()], numbers=[-1], outputs=("key_cell_begin",)),
        dict(parts=[part()], flags=4), dict(parts=[part()], flags=8 | N.GX_BUCKET_ALL_DIGITS), dict(parts=[], flags=0x80000000),
        # gx_group_lines' own
        dict(parts=None, n_parts=1), dict(parts=[part(reserved=1)]),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]),
        dict(parts=[part(extraction=1)]), dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(), part()]),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    # the order: gx_group_lines' refusals first, then number_groups, the number group, the width, cell_stats, outputs without a number
    order = [(dict(parts=[part(key_group=1)], numbers_null=True, width=0, flags=4), "unknown flag bits"),
             (dict(parts=[part(key_group=1)], numbers_null=True, width=0), "key_group"),
             (dict(parts=[part()], numbers_null=True, width=0, outputs=("cell_stats",)), "number_groups is NULL"),
             (dict(parts=[part()], numbers=[7], width=0, outputs=("cell_stats",)), "number group is neither -1 nor one of its extraction's"),
             (dict(parts=[part()], numbers=[-1], width=0, outputs=("cell_stats",)), "width below 1"),
             (dict(parts=[part()], numbers=[-1], outputs=("cell_stats", "cell_key")), "cell_stats without a value_group"),
             (dict(parts=[part()], numbers=[-1], outputs=("cell_key",), max_cells=2 ** 31), "every part's number group is -1")]
    for kw, words in order:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    limit = [dict(parts=[part()], max_cells=2 ** 30 + 1), dict(parts=[], max_cells=2 ** 40), dict(parts=[part()] * 65, numbers=[0] * 65),
             dict(parts=[part()], max_keys=2 ** 30 + 1)]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[], outputs=every_output), dict(parts=[], numbers_null=True), dict(parts=[part()]), dict(parts=[part()], outputs=every_output),
            dict(parts=[part()], series=False), dict(parts=[part()], numbers=[-1]), dict(parts=[part()], numbers=[-1], series=False),
            dict(parts=[part(value_group=0), part(extraction=2, key_group=1, value_group=0)], numbers=[-1, 2], outputs=every_output + ("cell_stats",)),
            dict(parts=[part(extraction=2, key_group=2, value_group=2)], numbers=[2]),                       # one group may be key, number and value
            dict(parts=[part()], max_cells=0), dict(parts=[part()], max_cells=2 ** 30),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BUCKET_ALL_DIGITS | N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], width=2 ** 63 - 1, origin=INT64_MIN), dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1),
            dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_series(data, offsets, ids, caps, [("gamma", "z", 0)], 60)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_series(bytes(text), [("alpha", "x", "x", "x")], 5, where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.group_series(data, offsets, ids, caps, [("alpha", "x", "x")], 0)
    assert ei.value.code == N.GX_E_ARG and "width" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.group_series(data, offsets, ids, caps, [("alpha", "x", "x")], 1, max_cells=2 ** 30 + 1)
    assert ei.value.code == N.GX_E_LIMIT


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_series_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_series(h, None, off, 1, id_ptr, None, None, 0, None, 0, 1, None, 0, 0, None, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_series(None, None, 0, None, 0, None, 0, 1, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_group_series(g._h.ptr, None, 5, None, 0, None, 0, 1, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_series_parts_resolve_names_and_groups_and_a_text_origin():
    g = three_rules()
    both = g.series_parts([("alpha", "x", "x", "x"), (2, "z", 0)])
    p, numbers = both
    assert isinstance(p, GroupParts) and p.n == 2 and p.has_values
    assert decode_parts(both) == [(0, 0, 0, 0), (2, 2, -1, 0)]
    assert g.series_parts(both) is both
    assert decode_parts(g.series_parts([("gamma", 1, None), ("alpha", 0, "x", None)])) == [(2, 1, -1, -1), (0, 0, -1, 0)]
    assert g.series_parts([])[0].n == 0
    for spec in ([("alpha",)], [("alpha", "x")], [("alpha", "x", "x", "x", 1)], [("alpha", "x", "y")], [("alpha", "x", 1)], [("gamma", "y", "z")], [("gamma", "z", "y")],
                 [("delta", "x", "x")], [("alpha", "x", "x"), ("alpha", "x", None)], [("alpha", "x", "x")] * 65):
        with pytest.raises(ValueError):
            g.series_parts(spec)
    # a text origin is read under the number format of the FIRST part that has a number
    both = g.series_parts([("alpha", "x", None), ("gamma", 0, "z")])
    assert g._series_origin(both, 7) == 7 and g._series_origin(both, "-12") == -12
    g.set_number_format("gamma", "z", "iso8601", 3)
    assert g._series_origin(both, "2026-01-03T00:00:00Z") == 1767398400000
    for bad in ("x", "", 2 ** 63, 1.5, True, None):
        with pytest.raises(ValueError):
            g._series_origin(both, bad)
    with pytest.raises(ValueError):
        g._series_origin(g.series_parts([("alpha", "x", None)]), "1")
    assert g._series_origin(g.series_parts([("alpha", "x", None)]), 5) == 5


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def series_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("series") / "series_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "series_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def test_sizes(series_exe):
    assert run_cases(series_exe, ["Z"]) == ["352 64 %d" % 2 ** 30]


def test_cell_word_round_trips_at_the_ends(series_exe):
    top = 2 ** 31 - 1
    pairs = [(0, 0), (0, top), (top, 0), (top, top), (1, 0), (0, 1), (5, 7)]
    got = run_cases(series_exe, ["C %d " % len(pairs) + " ".join("%d %d" % p for p in pairs)])[0].split()
    assert got == ["%d:%d:%d" % (cell_word(k, b), k, b) for k, b in pairs]
    words = [cell_word(k, b) for k, b in pairs]
    assert min(words) == 1 and max(words) < 2 ** 63 and len(set(words)) == len(pairs)
    assert all(cell_kslot(w) == k and cell_bslot(w) == b for w, (k, b) in zip(words, pairs))


@pytest.mark.parametrize("n_buckets", [1, 2 ** 30])
def test_sort_word_is_strictly_monotone_in_key_and_rank(series_exe, n_buckets):
    ranks = sorted(r for r in {0, 1, n_buckets // 2, n_buckets - 2, n_buckets - 1} if 0 <= r < n_buckets)
    keys = [0, 1, 2, 2 ** 30 - 2, 2 ** 30 - 1]
    triples = [(k, r, n_buckets) for k in keys for r in ranks]           # ascending in (key, rank)
    got = [int(x) for x in run_cases(series_exe, ["S %d " % len(triples) + " ".join("%d %d %d" % t for t in triples)])[0].split()]
    assert got == [sort_word(*t) for t in triples]
    assert all(a < b for a, b in zip(got, got[1:])) and got[-1] < 2 ** 60
    assert got[-1] == 2 ** 30 * n_buckets - 1


def test_the_digit_count(series_exe):
    products = [1, 63, 64, 65, 4095, 4096, 4097, 2 ** 60 - 1, 2 ** 60]
    pairs = [(p, 1) for p in products] + [(1, p) for p in products if p <= 2 ** 30] + [(0, 0), (0, 5), (7, 9), (8, 8), (13, 5), (2 ** 30, 2 ** 30)]
    got = [int(x) for x in run_cases(series_exe, ["D %d " % len(pairs) + " ".join("%d %d" % p for p in pairs)])[0].split()]
    assert got == [series_digits(*p) for p in pairs]
    assert [series_digits(p, 1) for p in (1, 63, 64, 65, 4096, 2 ** 60 - 1)] == [0, 1, 1, 2, 2, 10]
    # the digits cover the largest sort word there can be
    for k, b in pairs:
        if k * b:
            assert sort_word(k - 1, b - 1, b) < 64 ** max(series_digits(k, b), 0) or k * b == 1


def probe(table, slots, word, weak):
    s = bucket_hash(word, weak) & (slots - 1)
    for _ in range(slots):
        if s not in table:
            table[s] = word
        if table[s] == word:
            return s
        s = (s + 1) & (slots - 1)
    return None


@pytest.mark.parametrize("weak", [0, 1])
@pytest.mark.parametrize("slots,n_keys,n_buckets", [(64, 3, 5), (64, 6, 12), (64, 1, 70), (128, 9, 9), (256, 40, 7)])
def test_find_or_insert_over_both_tables_against_the_python_probing(series_exe, weak, slots, n_keys, n_buckets):
    rng = np.random.default_rng(slots + n_keys)
    lines = [(int(rng.integers(0, n_keys)) * 7 % (2 ** 31), int(rng.integers(-n_buckets // 2, n_buckets // 2 + 1)) * 1000 - 3) for _ in range(400)]
    row = "T %d %d %d " % (weak, slots, len(lines)) + " ".join("%d %d" % l for l in lines)
    out = run_cases(series_exe, [row])[0]
    per_line, btext, ctext = [t.strip() for t in out.split("|")]
    bt, ct, want = {}, {}, []
    for kslot, bucket in lines:
        bslot = probe(bt, slots, word_of(bucket), bool(weak))
        if bslot is None:
            want.append("full:full")
            continue
        cslot = probe(ct, slots, cell_word(kslot, bslot), bool(weak))
        want.append("%d:%s" % (bslot, "full" if cslot is None else cslot))
    assert per_line.split() == want
    assert btext.split() == ["%d:%d" % (s, bt[s]) for s in sorted(bt)] and ctext.split() == ["%d:%d" % (s, ct[s]) for s in sorted(ct)]
    assert len(bt) <= len(ct) or "full" in out          # distinct buckets never exceed distinct cells
    if (slots, n_keys, n_buckets) == (64, 6, 12):
        assert any(w.endswith(":full") for w in want)    # 78 cells do not fit 64 slots: "full" is reported, and nothing is probed past the table
    assert all(0 < w <= M64 for w in ct.values())


# ---------------------------------------------------------------------------
# the numpy restatement the large GPU case relies on
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,width,origin", [(1, 300, 50_000, 0), (2, 500, 7_000, 1_000_000), (3, 64, 10 ** 9, 0), (4, 200, 1, -5)])
def test_the_numpy_restatement_against_the_oracle(seed, n, width, origin):
    key, v, matched = draw(n, seed, span=400_000)
    data, offsets, ids, caps = digits_batch(key, v, matched)
    want = group_series(data, offsets, ids, caps, [(0, 0, -1, 1)], origin, width, [], 1)
    got = np_series(key, v, matched, origin, width)
    for name, dtype in SERIES_FIELDS:
        assert got[name].dtype == dtype and got[name].tolist() == want[name], name
    assert want["totals"]["celled"] == int(matched.sum()) and want["totals"]["n_cells"] > 1
