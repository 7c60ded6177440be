"""GPU tests of gx_capture_stats / gx_text_capture_stats: what the lines of a finished batch captured as numbers, summarised.

Expected values come from tests/stats_oracle.py -- the value sliced out of the line with the capture offsets, where_oracle.parse_long,
Python's integers for the sum, bisect for the bucket -- and everything is compared exactly.  Most batches are fabricated against
handles of K identical, trivial extractions: a line is its value, its capture row (0, length), its id chosen here; the end-to-end
cases take ids and rows from gx_extract_batch."""
import ctypes as C
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from stats_oracle import SUM_SEQUENCES, capture_stats, decode_measures, same, split128
from where_oracle import INT64_MAX, INT64_MIN, INT_TABLE, decode_terms, unpack

pytestmark = pytest.mark.gpu

PUT, GET, OTHER = 0, 1, 2  # workloads.readme3_definition: the extractions' indices; groups timestamp, verb, timeTakenInMsec, path
K3 = 3
EDGES = [10, 100, 500, 1000]
GRID_LINES = 2048 * 256    # gx_stats.hip: lines of one trip of the grid stride


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, measures, where=None, utf8=None):
    """capture_stats against the restatement, every field; returns what the call returned."""
    m = gorp.measures(measures)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = capture_stats(data, offsets, ids, caps, decode_measures(m), decode_terms(terms), gorp.num_extractions)
    got = gorp.capture_stats(data, offsets, ids, caps, m, where=terms, utf8=utf8)
    same(got, want)
    return got


def plain(stats):
    return [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in stats]


_handles = {}


def trivial_handle(K, groups=1):
    """K identical extractions `a(.*)...`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups].num_extractions == K and _handles[K, groups].max_groups == groups
    return _handles[K, groups]


def csr(lines, dtype=np.uint8, offsets_dtype=np.uint32):
    """lines: sequences of code units"""
    offsets = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(offsets_dtype)
    data = np.array([u for ln in lines for u in ln], dtype=dtype)
    return data, offsets


def values_batch(values, ids, dtype=np.uint8):
    """a line is its value: caps (0, length)"""
    data, offsets = csr(values, dtype=dtype)
    caps = np.array([[0, len(v)] for v in values], np.int32).reshape(len(values), 2)
    return data, offsets, np.asarray(ids, np.int32), caps


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def in_format(ids, caps, fmt):
    """(ids, rows) as capture_stats takes them: int32 ids and dense rows, or u16 / u8 result rows"""
    return (ids, caps) if fmt == "int32" else (pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8), None)


def raw_call(gorp, data, offsets, ids, caps, measures, terms_ptr=None, n_terms=0, **kw):
    """gx_capture_stats itself on host arrays; returns (rc, stats array, hist)."""
    m = gorp.measures(measures)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    stats = (N.gx_measure_stats * max(1, m.n))()
    hist = np.zeros(m.n_bins, np.uint64)
    rc = N.lib().gx_capture_stats(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, len(offsets) - 1, ids.ctypes.data if ids.size else None,
                                  None if caps is None or not caps.size else caps.ctypes.data, m.array, m.n, terms_ptr, n_terms, stats, hist.ctypes.data, C.byref(o))
    return rc, Gorp._stats_result(m, stats, hist) if rc == N.GX_OK else None


# ---------------------------------------------------------------------------
# the README definition, extracted for real
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def readme():
    gorp = Gorp.construct(W.readme3_definition())
    n = 2000
    t_data, _, cat = W.readme3_lines(n, seed=5)
    data = t_data.numpy().copy()
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(ids, cat.numpy().astype(np.int32))
    assert (ids == GET).sum() > 500 and (ids == PUT).sum() > 500 and (ids == OTHER).sum() > 50 and (ids == -1).sum() > 10
    return gorp, data, offsets, ids, caps


README_MEASURES = [("GetRequest", "timeTakenInMsec", EDGES), ("PutRequest", "timeTakenInMsec", EDGES), ("GetRequest", "verb")]


@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_readme_definition_in_every_row_format_and_offset_width(readme, fmt, offsets_dtype):
    gorp, data, offsets, ids, caps = readme
    offsets = offsets.astype(offsets_dtype)
    if fmt == "int32":
        id_col, rows = ids, caps
    else:
        id_col, rows = gorp.extract_batch(data, offsets, compact=1 if fmt == "u16" else 2)[0], None
        assert np.array_equal(id_col, pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8))
    get, put, verb = check(gorp, data, offsets, id_col, rows, README_MEASURES)
    assert get["lines"] == get["numbers"] == (ids == GET).sum() and put["numbers"] == (ids == PUT).sum()
    assert get["unset"] == get["not_numbers"] == 0 and (get["hist"] > 20).all() and get["min"] >= 0 and get["max"] <= 9999
    assert verb["lines"] == verb["not_numbers"] == get["lines"] and verb["numbers"] == 0 and verb["min"] is None and verb["max"] is None and verb["sum"] == 0
    # the caller's loop, in Python: metrics.record(Long.parseLong(r.asMap().get("timeTakenInMsec")))
    took = [int(bytes(data[int(offsets[i]) + caps[i, 4]:int(offsets[i]) + caps[i, 5]])) for i in np.flatnonzero(ids == GET)]
    assert get["sum"] == sum(took) and get["min"] == min(took) and get["max"] == max(took)
    assert get["hist"].tolist() == [sum(1 for v in took if lo <= v < hi) for lo, hi in zip([-1] + EDGES, EDGES + [10 ** 9])]


# ---------------------------------------------------------------------------
# the classes: numbers, values that are none, unset groups, pairs that name no value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_classes_integer_table_unset_groups_and_invalid_pairs(fmt):
    gorp = trivial_handle(3)
    lines, caps, ids = [], [], []
    for k in (0, 2, 1):
        for v in INT_TABLE:
            lines += [v, b"x" + v + b"9"]                     # the value alone, and between units that would change the number
            caps += [[0, len(v)], [1, 1 + len(v)]]
            ids += [k, k]
        for pair in ((-1, -1), (-1, 3), (3, 2), (0, 6), (5, 6), (6, 6), (0, 5), (5, 5), (2, 4), (0, 0)):   # the line is b"12345"
            lines.append(b"12345")
            caps.append(list(pair))
            ids.append(k)
    lines.append(b"777")                                      # (the last line: "beyond the line" above stays inside the buffer)
    caps.append([0, 3])
    ids.append(0)
    data, offsets = csr(lines)
    ids, caps = np.array(ids, np.int32), np.array(caps, np.int32)
    id_col, rows = in_format(ids, caps, fmt)
    a, b = check(gorp, data, offsets, id_col, rows, [(0, 0, [0, 100]), (2, 0)])
    assert a["unset"] == 6 and b["unset"] == 6                # (-1, -1), (-1, 3), (3, 2), (0, 6), (5, 6), (6, 6)
    # 7 of the table's 16 values are numbers, each given twice; (0, 5) and (2, 4) are numbers, (5, 5) and (0, 0) empty values; and "777"
    assert a["numbers"] == 2 * 7 + 2 + 1 and a["not_numbers"] == 2 * 9 + 2 and b["numbers"] == a["numbers"] - 1
    assert a["min"] == INT64_MIN and a["max"] == INT64_MAX


def test_pairs_that_name_no_value_are_unset_one_by_one():
    gorp = trivial_handle(1)
    pairs = [(-1, -1), (-1, 3), (3, 2), (0, 6), (5, 6), (6, 6), (2 ** 31 - 1, 2 ** 31 - 1), (0, 2 ** 31 - 1), (-2 ** 31, 0), (0, 5), (5, 5), (2, 4)]
    for fmt in ("int32", "u16", "u8"):
        for b, e in pairs:
            if fmt != "int32" and not -1 <= min(b, e) <= max(b, e) < 250:
                continue
            data, offsets = csr([b"12345", b"6"])
            ids, caps = np.array([0, 0], np.int32), np.array([[b, e], [0, 1]], np.int32)
            id_col, rows = in_format(ids, caps, fmt)
            got = check(gorp, data, offsets, id_col, rows, [(0, 0)])[0]
            inside = 0 <= b <= e <= 5
            assert got["unset"] == (0 if inside else 1) and got["lines"] == 2
            assert got["numbers"] == (2 if inside and e > b else 1) and got["not_numbers"] == (1 if inside and e == b else 0)


# ---------------------------------------------------------------------------
# sums that leave int64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["up", "down", "mixed"])
def test_128_bit_sums(name):
    gorp = trivial_handle(2)
    values = [str(v).encode() for count, v in SUM_SEQUENCES[name] for _ in range(count)]
    assert len(values) == 70000
    np.random.default_rng(3).shuffle(values)
    ids = np.zeros(len(values), np.int32)
    ids[::7] = 1
    data, offsets, ids, caps = values_batch(values, ids)
    a, b = check(gorp, data, offsets, ids, caps, [(0, 0, [-1, 0, 1]), (1, 0)])
    total = sum(int(v) for v in values)
    assert a["sum"] + b["sum"] == total and not INT64_MIN <= a["sum"] <= INT64_MAX
    assert split128(a["sum"])[0] not in (0, -1) or name == "mixed"
    rc, raw = raw_call(gorp, data, offsets, ids, caps, [(0, 0)])
    assert rc == N.GX_OK and raw[0]["sum"] == a["sum"]


# ---------------------------------------------------------------------------
# histograms
# ---------------------------------------------------------------------------
EDGE_SETS = [[], [0], [INT64_MIN], [INT64_MAX], [INT64_MIN, INT64_MAX], [INT64_MIN, -1, 0, 1, INT64_MAX], EDGES, list(range(-320, 320, 10)),
             [INT64_MIN + 3 * j for j in range(32)] + [INT64_MAX - 3 * j for j in range(31, -1, -1)], [7 * j * j * j for j in range(-31, 32)]]


def probes(edges):
    out = {INT64_MIN, -1, 0, 1, INT64_MAX}
    for e in edges:
        out |= {v for v in (e - 1, e, e + 1) if INT64_MIN <= v <= INT64_MAX}
    return sorted(out)


def test_histogram_on_below_and_above_every_edge():
    K = len(EDGE_SETS)
    gorp = trivial_handle(K, groups=2)
    assert sorted(len(e) for e in EDGE_SETS)[:2] == [0, 1] and sorted(len(e) for e in EDGE_SETS)[-2:] == [64, 64]
    values, ids = [], []
    for k, edges in enumerate(EDGE_SETS):
        for v in probes(edges):
            values.append(str(v).encode())
            ids.append(k)
    order = np.random.default_rng(11).permutation(len(values))
    values, ids = [values[j] for j in order], [ids[j] for j in order]
    data, offsets = csr(values)
    caps = np.array([[0, len(v), 1, len(v)] for v in values], np.int32)      # group 1: the value without its first unit
    ids = np.array(ids, np.int32)
    got = check(gorp, data, offsets, ids, caps, [(k, 0, edges) for k, edges in enumerate(EDGE_SETS)])
    for k, edges in enumerate(EDGE_SETS):
        assert got[k]["numbers"] == len(probes(edges)) and len(got[k]["hist"]) == len(edges) + 1
        assert (got[k]["hist"][1:] > 0).all() and (got[k]["hist"][0] > 0) == (not edges or edges[0] > INT64_MIN)   # (nothing lies below INT64_MIN)
    # two measures on the same group with different edges, two groups of one extraction, given in any order
    spec = [(6, 0, EDGES), (7, 1, [0, 50]), (6, 0, [0]), (6, 1, EDGES), (7, 0, list(range(-320, 320, 10))), (6, 0), (0, 1)]
    got = check(gorp, data, offsets, ids, caps, spec)
    assert got[0]["numbers"] == got[2]["numbers"] == got[5]["numbers"] and got[0]["sum"] == got[2]["sum"] and got[3]["sum"] != got[0]["sum"]
    assert got[3]["not_numbers"] > 0 and got[5]["hist"].tolist() == [got[5]["numbers"]]


def test_64_measures_of_16_edges_and_the_refusal_at_1025():
    gorp = trivial_handle(10)
    rng = np.random.default_rng(4)
    n = 5000
    values = [str(int(v)).encode() for v in rng.integers(-50, 400, n)]
    data, offsets, ids, caps = values_batch(values, rng.integers(-2, 10, n))
    spec = [(j % 10, 0, [j + 20 * i for i in range(16)]) for j in range(64)]
    got = check(gorp, data, offsets, ids, caps, spec)
    assert len(got) == 64 and all(len(s["hist"]) == 17 and s["numbers"] > 300 for s in got)
    m = gorp.measures(spec)
    e17 = np.arange(17, dtype=np.int64)
    m.array[0].edges, m.array[0].n_edges, m.edges[0] = e17.ctypes.data, 17, e17
    with pytest.raises(GorpError) as ei:
        gorp.capture_stats(data, offsets, ids, caps, m)
    assert ei.value.code == N.GX_E_LIMIT and "1024" in ei.value.message


# ---------------------------------------------------------------------------
# wave shapes
# ---------------------------------------------------------------------------
def test_wave_shapes():
    gorp = trivial_handle(64)
    rng = np.random.default_rng(9)
    ids = np.concatenate([np.full(64, 5), np.arange(64), np.tile([3, 40], 32), np.full(64, -1), rng.permutation(64), np.tile([-2, 63, 0], 30)]).astype(np.int32)
    values = [str(int(v)).encode() for v in rng.integers(-1000, 1000, len(ids))]
    values[7], values[70], values[130] = b"", b"+", b"12a"
    data, offsets, ids, caps = values_batch(values, ids)
    caps[9] = caps[100] = caps[131] = -1
    everywhere = [(k, 0, [k - 32]) for k in range(64)]
    got = check(gorp, data, offsets, ids, caps, everywhere)
    assert got[5]["lines"] == 64 + 2 and got[3]["lines"] == 32 + 2 and got[5]["not_numbers"] == 1 and got[5]["unset"] == 1
    got = check(gorp, data, offsets, ids, caps, [(40, 0, EDGES), (3, 0), (3, 0, [0])])
    assert got[0]["lines"] == 32 + 2 and got[1]["numbers"] == got[2]["numbers"]
    # no line of the batch has a measure
    got = check(gorp, data, offsets, np.full(len(ids), -1, np.int32), caps, everywhere)
    assert all(s["lines"] == 0 and s["sum"] == 0 and s["min"] is None for s in got)
    got = check(gorp, data, offsets, np.where(ids == 5, 6, ids).astype(np.int32), caps, [(5, 0, EDGES)])
    assert got[0]["lines"] == 0 and got[0]["hist"].tolist() == [0] * 5


# ---------------------------------------------------------------------------
# sizes: lines, extractions
# ---------------------------------------------------------------------------
def four_byte_lines(n, K, measured, seed, dense_tail=1000, share=0.03):
    """n lines of 4 bytes; few lines of the measured extractions except among the last `dense_tail`, where every line is one."""
    rng = np.random.default_rng(seed)
    others = np.array([k for k in {0, K // 2, K - 1, 1 % K} if k not in measured] + [-1, -2, -1 - K], np.int32)
    ids = rng.choice(others, n)
    hit = rng.random(n) < share
    hit[max(0, n - dense_tail):] = True
    ids[hit] = rng.choice(np.array(measured, np.int32), int(hit.sum()))
    data = rng.integers(0x30, 0x3A, 4 * n, dtype=np.uint8)
    data[rng.random(4 * n) < 0.03] = ord("-")
    offsets = (np.arange(n + 1, dtype=np.uint64) * 4).astype(np.uint32)
    caps = np.tile(np.array([0, 4], np.int32), (n, 1))
    caps[rng.random(n) < 0.1] = -1
    caps[rng.random(n) < 0.1, 0] = 2
    return data, offsets, ids.astype(np.int32), caps


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, GRID_LINES - 1, GRID_LINES, GRID_LINES + 1])
def test_line_counts_around_wave_workgroup_and_grid_boundaries(n):
    gorp = trivial_handle(3)
    data, offsets, ids, caps = four_byte_lines(n, 3, [0, 2], seed=n)
    a, b = check(gorp, data, offsets, ids, caps, [(0, 0, EDGES), (2, 0, [-5, 5000])])
    assert a["lines"] + b["lines"] >= min(n, 1000)
    if n >= 64:
        assert a["numbers"] and a["unset"] and a["not_numbers"] and b["numbers"]
    if n > GRID_LINES:
        assert ids[-1] in (0, 2)                                # (the line of the second trip has a measure)
        tail = check(gorp, data, offsets[GRID_LINES:] , ids[GRID_LINES:], caps[GRID_LINES:], [(0, 0, EDGES), (2, 0, [-5, 5000])])
        assert tail[0]["lines"] + tail[1]["lines"] == 1


@pytest.mark.parametrize("K", [1, 31, 32, 2048, 4097])
def test_extraction_counts_measures_on_the_first_and_the_last(K):
    gorp = trivial_handle(K)
    measured = sorted({0, K - 1})
    data, offsets, ids, caps = four_byte_lines(6000, K, measured, seed=K, share=0.3)
    got = check(gorp, data, offsets, ids, caps, [(k, 0, EDGES) for k in measured])
    assert all(s["numbers"] > 300 and s["unset"] > 30 and s["not_numbers"] > 30 for s in got)
    # ids beyond the extractions and exceptions of the measured ones add nothing
    ids2 = ids.copy()
    ids2[ids2 < 0] = -2
    ids2[::5] = K
    check(gorp, data, offsets, ids2, caps, [(K - 1, 0), (0, 0, [0])])


# ---------------------------------------------------------------------------
# terms
# ---------------------------------------------------------------------------
def test_terms_are_select_lines_where_then_stats(readme):
    gorp, data, offsets, ids, caps = readme
    matched = np.concatenate([np.ones(K3, np.uint8), np.zeros(K3 + 1, np.uint8)])
    specs = [[("GetRequest", "timeTakenInMsec", ">=", 500)],
             [("GetRequest", "timeTakenInMsec", "<", 500), ("PutRequest", "path", "contains", "a")],
             [("GetRequest", "path", "not contains", "a"), ("GetRequest", "timeTakenInMsec", ">", 9)],
             [("PutRequest", "verb", "==", "PUT"), ("OtherRequest", "verb", "!=", "POST")],
             [("GetRequest", "verb", "unset")]]
    without = check(gorp, data, offsets, ids, caps, README_MEASURES)
    for fmt in ("int32", "u8"):
        id_col, rows = (ids, caps) if fmt == "int32" else (gorp.extract_batch(data, offsets, compact=2)[0], None)
        for spec in specs:
            got = check(gorp, data, offsets, id_col, rows, README_MEASURES, where=spec)
            sel = gorp.select_lines_where(data, offsets, id_col, rows, spec, want=matched)
            sids, srows = (sel[3], sel[4]) if fmt == "int32" else (sel[3], None)
            again = check(gorp, sel[1], sel[2], sids, srows, README_MEASURES)
            assert plain(again) == plain(got)
            assert got[0]["lines"] < without[0]["lines"] or spec is specs[3]
        assert check(gorp, data, offsets, id_col, rows, README_MEASURES, where=specs[4])[0]["lines"] == 0
    assert plain(check(gorp, data, offsets, ids, caps, README_MEASURES, where=specs[3])[0:1]) == plain(without[0:1])   # (no term on GetRequest)
    # n_terms == 0 is passing no terms
    some = (N.gx_where_term * 1)()
    rc, a = raw_call(gorp, data, offsets, ids, caps, README_MEASURES, terms_ptr=some, n_terms=0)
    rc2, b = raw_call(gorp, data, offsets, ids, caps, README_MEASURES, terms_ptr=None, n_terms=0)
    assert rc == rc2 == N.GX_OK and plain(a) == plain(b) == plain(without)
    # no measures: legal, nothing to deliver
    assert gorp.capture_stats(data, offsets, ids, caps, []) == []
    assert gorp.capture_stats(data, offsets, ids, caps, [], where=specs[0]) == []


# ---------------------------------------------------------------------------
# code units: UTF-16, UTF-8 bytes
# ---------------------------------------------------------------------------
def test_utf16_units_and_a_digit_that_is_not_ascii():
    gorp = trivial_handle(2)
    lines = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31, 0x32], [0x131, 0x32], [0x2D, 0x37], [0x2D, 0xFF17], [0x416], [0x16], [0x0416, 0x31], [], [0x2B, 0x39, 0x39]]
    data, offsets = csr(lines * 2, dtype=np.uint16)
    ids = np.array([0] * len(lines) + [1] * len(lines), np.int32)
    caps = np.array([[0, len(ln)] for ln in lines * 2], np.int32)
    a, b = check(gorp, data, offsets, ids, caps, [(0, 0, [0, 50]), (1, 0)])
    assert (a["numbers"], a["not_numbers"], a["sum"], a["min"], a["max"]) == (4, 8, 1 + 12 - 7 + 99, -7, 99) and a["hist"].tolist() == [1, 2, 1]
    got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], where=[(1, 0, "startswith", "1"), (0, 0, "not contains", "１")])
    assert got[0]["lines"] == 10 and got[1]["lines"] == 3 and got[1]["numbers"] == 2
    for fmt in ("u16", "u8"):
        id_col, _ = in_format(ids, caps, fmt)
        assert plain(check(gorp, data, offsets, id_col, None, [(0, 0, [0, 50]), (1, 0)])) == plain([a, b])
    # lines of the README definition as UTF-16
    gorp = Gorp.construct(W.readme3_definition())
    n = 600
    t_data, _, _ = W.readme3_lines(n, seed=8)
    data = t_data.numpy().astype(np.uint16)
    data[np.flatnonzero(data == ord("~"))[::3]] = 0x416
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    got = check(gorp, data, offsets, ids, caps, README_MEASURES, where=[("GetRequest", "path", "contains", "Ж")])
    assert 0 < got[0]["lines"] < (ids == GET).sum()


def test_utf8_bytes_with_lines_that_are_not_ascii():
    gorp = Gorp.construct(W.readme3_definition())
    rng = random.Random(12)
    lines = []
    for j in range(1500):
        verb = rng.choice(["GET", "GET", "PUT", "POST"])
        lines.append("[%d]: %s %dms /%s%s" % (rng.randrange(1, 10 ** 9), verb, rng.choice([7, 499, 500, rng.randrange(0, 100000)]), rng.choice(["v1/", "café/", "Ж€/"]),
                                              "x" * rng.randrange(0, 30)))
    data, offsets = lines_to_csr([ln.encode("utf-8") for ln in lines])
    assert (data >= 0x80).any()
    ids, caps = gorp.extract_batch(data, offsets, utf8="bytes")
    assert (ids == GET).sum() > 500
    got = check(gorp, data, offsets, ids, caps, README_MEASURES, utf8="bytes")
    assert got[0]["numbers"] == (ids == GET).sum()
    got = check(gorp, data, offsets, ids, caps, README_MEASURES, where=[("GetRequest", "path", "contains", "café")], utf8="bytes")
    assert 100 < got[0]["numbers"] < (ids == GET).sum() - 100 and got[1]["numbers"] == (ids == PUT).sum()
    # utf8 = 2 (offsets in units over a byte buffer) is refused
    rc, _ = raw_call(gorp, data, offsets, ids, caps, README_MEASURES, utf8=2)
    assert rc == N.GX_E_ARG and "utf8" in N.last_error()
    rc, _ = raw_call(gorp, data, offsets, ids, caps, README_MEASURES, no_sync=1)
    assert rc == N.GX_E_ARG and "no_sync" in N.last_error()


# ---------------------------------------------------------------------------
# device buffers: alignment, the end of the allocation, stream order, determinism
# ---------------------------------------------------------------------------
def test_device_buffers_at_every_misalignment_end_with_the_last_capture():
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n = 3000
    values = [str(int(v)).encode() for v in rng.integers(-10 ** 6, 10 ** 12, n)]
    values[-1] = b"9223372036854775807"                                       # the last capture ends at the buffer's last byte
    data, offsets, ids, caps = values_batch(values, rng.integers(-2, 4, n))
    ids[-1] = 3
    rows8 = pack(ids, caps, np.uint8)
    spec = [(3, 0, EDGES), (0, 0, [0]), (3, 0)]
    host = check(gorp, data, offsets, ids, caps, spec)
    assert plain(check(gorp, data, offsets, rows8, None, spec)) == plain(host) and host[0]["max"] == INT64_MAX
    d_off, d_ids, d_caps = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    for mis in range(16):
        src = torch.empty(mis + len(data), dtype=torch.uint8, device="cuda")     # sized exactly: the batch ends where the tensor ends
        src[mis:] = torch.from_numpy(data).cuda()
        got = gorp.capture_stats_device(src.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), spec)
        assert plain(got) == plain(host)
        d_rows = torch.empty(mis + rows8.size, dtype=torch.uint8, device="cuda")
        d_rows[mis:] = torch.from_numpy(rows8.reshape(-1)).cuda()
        got = gorp.capture_stats_device(src.data_ptr() + mis, d_off.data_ptr(), n, d_rows.data_ptr() + mis, None, spec, compact=2,
                                        where=[(3, 0, ">=", -10 ** 7)])
        assert plain(got) == plain(host)
    # dense ids without capture rows: refused on a handle with a device too
    with pytest.raises(GorpError) as ei:
        gorp.capture_stats_device(src.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), None, spec)
    assert ei.value.code == N.GX_E_ARG


def test_the_call_follows_a_no_sync_batch_on_its_stream_and_two_runs_are_the_same_bits():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 60000, 200
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.full((n, width), 0x55, dtype=torch.uint8, device="cuda")       # ids nobody wrote: outcome 2K + 1
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    where = [("GetRequest", "timeTakenInMsec", ">=", 500)]
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True, compact=2,
                                  line_bytes_hint=L)
        got = gorp.capture_stats_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, README_MEASURES, where=where, compact=2,
                                        stream=stream.cuda_stream)
        # a no_sync selection leaves its copy pass reading the handle's select workspace; the stats call has buffers of its own
        k, nbytes = gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, "matched-by-terms", where, compact=2,
                                                   stream=stream.cuda_stream)
        again = gorp.capture_stats_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, README_MEASURES, where=where, compact=2,
                                          stream=stream.cuda_stream)
    stream.synchronize()
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(unpack(h_rows)[0], cat.cpu().numpy().astype(np.int32))
    m = gorp.measures(README_MEASURES)
    want = capture_stats(h_data, h_off, h_rows, None, decode_measures(m), decode_terms(gorp.where_terms(where)), K3)
    same(got, want)
    assert plain(again) == plain(got) and got[0]["lines"] == k > 1000                 # two runs: the same bits
    for _ in range(3):
        assert plain(gorp.capture_stats_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, README_MEASURES, where=where, compact=2)) == plain(got)


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------
def text_lines(n, seed, utf8):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        verb = rng.choice(["GET"] * 4 + ["PUT"] * 3 + ["POST", "DELETE", "HEAD"])
        ms = rng.choice([rng.randrange(0, 10), rng.randrange(0, 1000), rng.randrange(0, 100000), 500, 499, 7]) if rng.random() < 0.9 else "007"
        path = "/" + rng.choice(["v1/", "v2/", "café/", "Ж€/"] if utf8 else ["v1/", "v2/", "api/v1/x", ""]) + "x" * rng.randrange(0, 40)
        line = "[%d]: %s %sms %s" % (rng.randrange(1, 10 ** 9), verb, ms, path)
        r = rng.random()
        if r < 0.08:
            line = line.replace("]: ", "]; ")                       # no extraction matches
        elif r < 0.14:
            line = line + "\x0bq"                                   # the automaton takes VT for \S, the capture regexp does not: the line raises
        elif r < 0.17:
            line = ""
        out.append(line)
    return out


@pytest.mark.parametrize("utf8", [False, True])
def test_text_capture_stats_is_split_extract_stats(utf8):
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in text_lines(3000, 21, utf8)]
    text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 777ms /tail"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
    assert (ids < -1).sum() > 50 and (ids == -1).sum() > 100
    wheres = [None, [("GetRequest", "timeTakenInMsec", ">=", 500)], [("GetRequest", "path", "contains", "café" if utf8 else "/v1/"), ("PutRequest", "timeTakenInMsec", "<", 500)]]
    for where in wheres:
        want = check(gorp, data, offsets, ids, caps, README_MEASURES, where=where, utf8="bytes" if utf8 else None)
        got, counts, n_lines = gorp.text_capture_stats(text, README_MEASURES, where=where, utf8=utf8)
        assert plain(got) == plain(want) and n_lines == len(raw) + 1
        assert np.array_equal(counts, gorp.text_select(text, "unmatched", utf8=utf8)[1]) and np.array_equal(counts, gorp.count_outcomes(ids))
        assert 0 < got[0]["lines"] and got[0]["max"] >= 777
    # no measures: counts and the line count alone; an empty text
    got, counts, n_lines = gorp.text_capture_stats(text, [], utf8=utf8)
    assert got == [] and n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids))
    got, counts, n_lines = gorp.text_capture_stats(b"", README_MEASURES, utf8=utf8)
    assert n_lines == 0 and counts.sum() == 0 and all(s["lines"] == 0 and s["min"] is None and s["sum"] == 0 for s in got)


@pytest.mark.parametrize("n", [0, 1, 65])
def test_text_form_from_host_buffers_and_device_pointers(n):
    """the same text once from a host buffer and once from a device pointer: equal stats, histogram, counts and line count, and the
    stats are those of the GET lines (every third line; among 65 lines one is empty and one matches nothing)"""
    from twin_buffers import twins
    gorp = Gorp.construct(W.readme3_definition())
    lines = ["[%d]: %s %dms /p/%d" % (i, ("GET", "PUT", "POST")[i % 3], 10 * i, i % 7) for i in range(n)]
    if n > 9:
        lines[5], lines[9] = "", "nothing here"
    text = np.frombuffer("".join(l + "\n" for l in lines).encode(), np.uint8)
    text16 = np.zeros((text.size + 15) // 16 * 16 + 16, np.uint8)       # (a device text is 16-byte aligned: torch's allocations are)
    text16[:text.size] = text
    v = np.array([10 * i for i in range(n) if i % 3 == 0 and i != 9], np.int64)     # (no value lies on an edge)
    for where, keep in ((None, v), ([("GetRequest", "timeTakenInMsec", ">=", 300)], v[v >= 300])):
        def call(b, device_pointers):
            stats, counts, n_lines = gorp.text_capture_stats_device(b.put(text16), text.size, README_MEASURES, where, device_pointers=device_pointers)
            return plain(stats), counts.tolist(), n_lines
        (stats, counts, n_lines), _ = twins(call)
        assert n_lines == n and sum(counts) == n and counts[gorp.num_extractions] == (2 if n > 9 else 0)      # (unmatched: the empty line and "nothing here")
        get = stats[0]
        assert get["lines"] == get["numbers"] == len(keep) and get["unset"] == get["not_numbers"] == 0 and get["sum"] == int(keep.sum())
        assert (get["min"], get["max"]) == ((int(keep.min()), int(keep.max())) if len(keep) else (None, None))
        assert get["hist"] == np.bincount(np.searchsorted(EDGES, keep), minlength=len(EDGES) + 1).tolist()
        assert stats[2]["lines"] == len(keep) and stats[2]["numbers"] == 0 and stats[2]["not_numbers"] == len(keep)   # ("GET" is no number)


# ---------------------------------------------------------------------------
# a batch that lives on the device, against torch's integer reductions
# ---------------------------------------------------------------------------
def test_200k_lines_on_the_device_against_torch():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 200000, 200
    data, offsets, cat = W.readme3_lines(n, seed=12, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    caps = torch.empty((n, 2 * gorp.max_groups), dtype=torch.int32, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
    assert torch.equal(ids, cat.to(torch.int32))
    got = gorp.capture_stats_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), README_MEASURES)
    slow = gorp.capture_stats_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), README_MEASURES,
                                     where=[("GetRequest", "timeTakenInMsec", ">=", 500)])
    edges = torch.tensor(EDGES, dtype=torch.int64, device="cuda")
    pow10 = torch.tensor([1, 10, 100, 1000], dtype=torch.int64, device="cuda")
    for k, s in ((GET, got[0]), (PUT, got[1])):
        sel = ids == k
        b, e = caps[sel, 4].to(torch.int64), caps[sel, 5].to(torch.int64)
        nd = e - b
        assert int(nd.min()) >= 1 and int(nd.max()) <= 4
        j = torch.arange(4, device="cuda")[None, :]
        digit = data.view(n, L)[sel].gather(1, (b[:, None] + j).clamp(max=L - 1)).to(torch.int64) - 48
        place = pow10[(nd[:, None] - 1 - j).clamp(min=0)]
        v = (digit * place * (j < nd[:, None])).sum(1)
        assert s["lines"] == s["numbers"] == int(sel.sum()) and s["unset"] == s["not_numbers"] == 0
        assert (s["sum"], s["min"], s["max"]) == (int(v.sum()), int(v.min()), int(v.max()))
        assert s["hist"].tolist() == torch.bincount(torch.bucketize(v, edges, right=True), minlength=5).tolist()
        if k == GET:
            big = v[v >= 500]
            assert (slow[0]["numbers"], slow[0]["sum"], slow[0]["min"]) == (int(big.numel()), int(big.sum()), int(big.min()))
            assert slow[0]["hist"].tolist() == torch.bincount(torch.bucketize(big, edges, right=True), minlength=5).tolist()
    assert plain(slow[1:2]) == plain(got[1:2]) and got[2]["not_numbers"] == got[0]["lines"]
