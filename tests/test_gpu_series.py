"""GPU tests of gx_group_series / gx_text_group_series: the lines of a batch counted and measured per (captured text, interval of a
captured number) -- the axis of occupied buckets, the cells ordered by (key number, bucket), every key's run of cells, the cell of every
line.

Expected values come from tests/series_oracle.py -- where_oracle / number_oracle / bucket_oracle.bucket_of for which lines count and what
their bucket is, a dict keyed by (key bytes, bucket) ordered by (key first line, bucket) -- and everything is compared bit for bit.  In
every case the key outputs and totals["group"] are compared byte for byte with gx_group_lines' on the same arguments, and the case runs
once more under GX_BUCKET_ALL_DIGITS and (up to 4 096 cells) under GX_GROUP_WEAK_HASH and under both, and must give the same bytes.  Most
batches are fabricated against handles of K identical, trivial extractions with three groups: a line is its key's text, its number's
text, its value's text and filler, its capture row made up here; the end-to-end case takes ids and rows from gx_extract_batch.  The large
shape is compared with a numpy restatement (np.unique over (line_key, bucket)), which tests/test_series_host.py compares with the oracle
on smaller draws of the same generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, parse_number
from number_oracle import KINDS
from series_oracle import NONE, SERIES_FIELDS, SERIES_TOTALS, batch, decode_parts, digits_batch, draw, group_series, np_series, same, series_digits
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG_LINES = int(re.search(r"constexpr uint32_t BUCKET_WG_LINES = (\d+);", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_bucket.hpp")).read()).group(1))
LDS_KEYS = int(re.search(r"GROUP_LDS_KEYS = (\d+);", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_group.hpp")).read()).group(1))
BLOCK = 2048                                                                                  # gx_scan.hpp's and the sort's block
P = [(0, 0, 1)]           # extraction 0: group 0 the key, group 1 the number
PV = [(0, 0, 1, 2)]       # ... and group 2 measured
KEY_FIELDS = ("key_units", "key_offsets", "first_line", "lines", "line_key")
FIELDS = tuple(name for name, _ in SERIES_FIELDS)


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, width, origin=0, where=None, utf8=None, formats=None, **kw):
    """group_series against the restatement, every field; the keys against group_lines on the same arguments, byte for byte; then under
    the test hooks, the same bytes.  Returns what the call returned."""
    both = gorp.series_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    fm = {key: (KINDS[kind], scale) for key, (kind, scale) in (formats or {}).items()}
    want = group_series(data, offsets, ids, caps, decode_parts(both), gorp._series_origin(both, origin), width, decode_terms(terms), gorp.num_extractions, fm)
    got = gorp.group_series(data, offsets, ids, caps, both, width, origin, where=terms, utf8=utf8, **kw)
    same(got, want)
    keys = gorp.group_lines(data, offsets, ids, caps, both[0], where=terms, utf8=utf8, max_keys=kw.get("max_keys"))
    assert got["totals"]["group"] == keys["totals"] and got["stats"] == keys["stats"] and got["keys"] == keys["keys"]
    assert {k: got["totals"][k] for k in keys["totals"]} == keys["totals"]
    for name in KEY_FIELDS:
        assert got[name].dtype == keys[name].dtype and got[name].tobytes() == keys[name].tobytes(), name
    hooks = [dict(all_digits=True)] + ([dict(weak_hash=True), dict(weak_hash=True, all_digits=True)] if want["totals"]["n_cells"] <= 4096 else [])
    for hook in hooks:
        again = gorp.group_series(data, offsets, ids, caps, both, width, origin, where=terms, utf8=utf8, **dict(kw, **hook))
        assert again["totals"] == got["totals"] and again["cell_stats"] == got["cell_stats"] and again["stats"] == got["stats"], hook
        for name in FIELDS + KEY_FIELDS:
            assert again[name].dtype == got[name].dtype and again[name].tobytes() == got[name].tobytes(), (hook, name)
    return got


_handles = {}


def trivial_handle(K, groups=3, tag=""):
    """K identical extractions `a(.*)(.*)(.*)`: a handle for ids and capture rows made up here (tag: a handle of its own, for number formats)."""
    if (K, groups, tag) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups, tag] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups, tag].num_extractions == K and _handles[K, groups, tag].max_groups == groups
    return _handles[K, groups, tag]


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def names(numbers):
    return [b"k%d" % int(k) for k in numbers]


# ---------------------------------------------------------------------------
# 1. what a cell is
# ---------------------------------------------------------------------------
def test_four_lines_two_keys_two_buckets_around_the_origin():
    gorp = trivial_handle(1)
    got = check(gorp, *batch([b"GET", b"PUT", b"GET", b"PUT"], [-1, 0, 59_999, -60_001]), P, 60_000)
    assert got["keys"] == [b"GET", b"PUT"] and got["bucket_number"].tolist() == [-2, -1, 0]
    assert got["cell_key"].tolist() == [0, 0, 1, 1] and got["cell_bucket"].tolist() == [1, 2, 0, 2] and got["cell_first_line"].tolist() == [0, 2, 3, 1]
    assert got["key_cell_begin"].tolist() == [0, 2, 4] and got["line_cell"].tolist() == [0, 3, 1, 2] and got["cell_lines"].tolist() == [1, 1, 1, 1]
    t = got["totals"]
    assert (t["n_cells"], t["n_buckets"], t["celled"], t["first_bucket"], t["last_bucket"], t["cells_exact"]) == (4, 3, 4, -2, 0, True)
    got = check(gorp, *batch([b"a", b"b", b"a", b"b"], [999, 1000, 1059, 939]), P, 60, origin=1000)        # the same four around another origin
    assert got["bucket_number"].tolist() == [-2, -1, 0] and got["cell_bucket"].tolist() == [1, 2, 0, 2]


def test_each_class_of_keyed_line_adds_up_and_a_part_without_a_number():
    gorp = trivial_handle(2)
    keys = [b"x", b"x", b"y", b"x", None, b"y", b"y", b"z", b"x", b"y"]
    numbers = [5, -2 ** 63, None, b"12x", 7, b"", 6, 8, 5, 5]
    ids = [0, 0, 0, 0, 0, 0, 1, 1, -1, 0]
    data, offsets, ids, caps = batch(keys, numbers, values=[1, 2, 3, 4, 5, 6, 7, None, 9, b"q"], lengths=[9] * 10, ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, 1, 2)], 1)
    t = got["totals"]
    assert (t["lines"], t["keyed"], t["unset"], t["celled"], t["number_unset"], t["not_numbers"], t["out_of_range"]) == (9, 8, 1, 4, 1, 2, 1)
    assert got["keys"] == [b"x", b"y", b"z"] and got["cell_key"].tolist() == [0, 1, 1, 2] and got["bucket_number"].tolist() == [5, 6, 8]
    assert got["line_cell"].tolist() == [0, NONE, NONE, NONE, NONE, NONE, 2, 3, NONE, 1]
    assert [s["numbers"] for s in got["cell_stats"]] == [1, 0, 1, 0] and got["cell_stats"][1]["not_numbers"] == 1 and got["cell_stats"][3]["unset"] == 1
    # number_groups = -1 for one of two parts: extraction 1's lines have a key and no number
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, None, 2)], 1)
    t = got["totals"]
    assert (t["keyed"], t["celled"], t["number_unset"]) == (8, 2, 3) and got["key_cell_begin"].tolist() == [0, 1, 2, 2] and got["keys"] == [b"x", b"y", b"z"]
    # no part at all, and no line at all: all zeros, key_cell_begin's one entry, no line has a cell
    got = check(gorp, data, offsets, ids, caps, [], 1)
    assert got["totals"]["n_cells"] == 0 and got["key_cell_begin"].tolist() == [0] and set(got["line_cell"].tolist()) == {NONE} and got["totals"]["cells_exact"]
    got = check(gorp, *batch([], []), P, 1)
    assert got["totals"]["n_cells"] == 0 and len(got["line_cell"]) == 0 and got["key_cell_begin"].tolist() == [0]
    got = check(gorp, *batch([b"a", b"b"], [None, b"x"]), P, 1)                               # keyed lines, none of them celled
    assert got["totals"]["n_cells"] == 0 and got["key_cell_begin"].tolist() == [0, 0, 0] and got["line_cell"].tolist() == [NONE, NONE]


# ---------------------------------------------------------------------------
# 2. one wave
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [1, 2, 7, 64])
def test_one_wave_of_64_lines(distinct):
    gorp = trivial_handle(1)
    i = np.arange(64)
    c = i % distinct
    got = check(gorp, *batch(names(c % 3), (c // 3 * 60 + 600).tolist(), values=(i * 5 - 100).tolist()), PV, 60)
    assert got["totals"]["n_cells"] == distinct and int(got["cell_lines"].sum()) == 64 and sum(s["numbers"] for s in got["cell_stats"]) == 64


def test_one_wave_two_keys_lane_by_lane_a_bucket_edge_and_the_three_branches_of_the_gather():
    gorp = trivial_handle(1)
    i = np.arange(64)
    got = check(gorp, *batch(names(i & 1), [600] * 64, values=i.tolist()), PV, 60)              # two keys alternating lane by lane in one bucket
    assert got["cell_lines"].tolist() == [32, 32] and got["totals"]["n_buckets"] == 1 and [s["sum"] for s in got["cell_stats"]] == [992, 1024]
    got = check(gorp, *batch(names([0] * 64), np.where(i <= 30, 659, 660).tolist(), values=i.tolist()), PV, 60)   # one key across a bucket edge
    assert got["cell_lines"].tolist() == [31, 33] and got["cell_first_line"].tolist() == [0, 31] and got["key_cell_begin"].tolist() == [0, 2]
    # cells whose lines carry zero, one and several numbers: key 0 none, key 1 one (not in its lowest lane), key 2 all
    values = [None if k == 0 else (77 if q == 40 else b"x") if k == 1 else q for q, k in enumerate((i % 3).tolist())]
    got = check(gorp, *batch(names(i % 3), [600] * 64, values=values), PV, 60)
    assert [s["numbers"] for s in got["cell_stats"]] == [0, 1, 21] and got["cell_stats"][1]["sum"] == 77 and got["cell_stats"][1]["min"] == 77
    assert got["cell_stats"][0]["unset"] == 22 and got["cell_stats"][1]["not_numbers"] == 20


# ---------------------------------------------------------------------------
# 3. and 4. workgroup edges and the workgroup's table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [WG_LINES - 1, WG_LINES, WG_LINES + 1, 2 * WG_LINES + 1])
def test_workgroup_edges_with_a_cell_spanning_the_edge(n):
    gorp = trivial_handle(1)
    i = np.arange(n)
    numbers = (i + 40) // 100 * 60                                                           # a bucket edge every 100 lines, none at a workgroup edge
    got = check(gorp, *batch(names(i % 2), numbers.tolist(), values=(i % 13).tolist()), PV, 60)
    assert got["totals"]["celled"] == n and int(got["cell_lines"].sum()) == n and got["totals"]["n_cells"] == 2 * len(set(numbers.tolist()))


@pytest.mark.parametrize("distinct", [LDS_KEYS + 1, 2 * LDS_KEYS + 1])
def test_more_cells_in_a_workgroup_than_its_lds_table_claims(distinct):
    gorp = trivial_handle(1)
    assert distinct <= WG_LINES
    rng = np.random.default_rng(distinct)
    block = np.concatenate([np.arange(distinct), rng.integers(0, distinct, WG_LINES - distinct)])    # one workgroup's lines: every cell at least once
    cell = np.concatenate([rng.permutation(block), rng.permutation(block), rng.permutation(block)[:100]])
    got = check(gorp, *batch(names(cell % 5), (cell // 5 * 10).tolist(), values=(cell % 97).tolist()), PV, 10)
    assert got["totals"]["n_cells"] == distinct and int(got["cell_lines"].sum()) == len(cell)


# ---------------------------------------------------------------------------
# 5. and 6. the scans' and the sorts' block edges, the digit boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("one_key", [False, True])
@pytest.mark.parametrize("n_cells", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_cell_counts_at_the_edges_of_a_scan_and_a_sort_block(n_cells, one_key):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n_cells)
    cell = rng.permutation(np.concatenate([np.arange(n_cells), rng.integers(0, n_cells, 300)]))
    keys, numbers = (np.zeros_like(cell), cell * 3 - 2000) if one_key else (cell % 7, cell // 7 * 3 - 200)
    got = check(gorp, *batch(names(keys), numbers.tolist()), P, 3, max_cells=n_cells)
    assert got["totals"]["n_cells"] == n_cells and int(got["cell_lines"].sum()) == n_cells + 300
    assert got["totals"]["n_buckets"] == (n_cells if one_key else (n_cells + 6) // 7)


@pytest.mark.parametrize("product", [63, 64, 65, 4095, 4096, 4097])
def test_the_cells_digit_plan_on_either_side_of_a_boundary(product):
    gorp = trivial_handle(1)
    n_keys, n_buckets = {63: (7, 9), 64: (8, 8), 65: (13, 5), 4095: (63, 65), 4096: (64, 64), 4097: (17, 241)}[product]
    assert n_keys * n_buckets == product and series_digits(n_keys, n_buckets) == (1 if product <= 64 else 2 if product <= 4096 else 3)
    rng = np.random.default_rng(product)
    # every key and every bucket at least once, the last key in the last bucket (the largest sort word), and a sparse rest
    k = np.concatenate([np.arange(n_keys), rng.integers(0, n_keys, n_buckets), [n_keys - 1], rng.integers(0, n_keys, 200)])
    b = np.concatenate([rng.integers(0, n_buckets, n_keys), np.arange(n_buckets), [n_buckets - 1], rng.integers(0, n_buckets, 200)])
    order = rng.permutation(len(k))
    got = check(gorp, *batch(names(k[order]), (b[order] * 10).tolist()), P, 10)
    assert got["totals"]["n_keys"] == n_keys and got["totals"]["n_buckets"] == n_buckets


# ---------------------------------------------------------------------------
# 7. order
# ---------------------------------------------------------------------------
def test_order_keys_by_first_line_buckets_ascending_and_an_empty_run():
    gorp = trivial_handle(1)
    # keys whose first lines descend while their buckets ascend: the later a key appears, the smaller its buckets
    keys = [b"late", b"mid", b"early", b"late", b"mid", b"early", b"mid"]
    numbers = [900, 500, 100, 800, 400, 0, 600]
    got = check(gorp, *batch(keys, numbers), P, 100)
    assert got["keys"] == [b"late", b"mid", b"early"] and got["cell_key"].tolist() == [0, 0, 1, 1, 1, 2, 2]
    assert got["bucket_number"][got["cell_bucket"]].tolist() == [8, 9, 4, 5, 6, 0, 1] and got["cell_first_line"].tolist() == [3, 0, 4, 1, 6, 5, 2]
    # a key with no cell between two keys with cells: an empty run
    got = check(gorp, *batch([b"a", b"b", b"c", b"a", b"b"], [5, b"x", 7, 9, None]), P, 1)
    assert got["key_cell_begin"].tolist() == [0, 2, 2, 3] and got["cell_key"].tolist() == [0, 0, 2]
    # a shuffled batch
    rng = np.random.default_rng(7)
    k, b = rng.integers(0, 9, 3000), rng.integers(-40, 40, 3000)
    got = check(gorp, *batch(names(k), (b * 1000 + rng.integers(0, 1000, 3000)).tolist(), values=rng.integers(-50, 50, 3000).tolist()), PV, 1000)
    word = got["cell_key"].astype(np.int64) * 100 + got["cell_bucket"]
    assert (np.diff(word) > 0).all() and (np.diff(got["cell_first_line"].astype(np.int64)) < 0).any() and (np.diff(got["bucket_number"]) > 0).all()


# ---------------------------------------------------------------------------
# 8. the tables and the capacities
# ---------------------------------------------------------------------------
OUTS = ("bucket_number", "cell_key", "cell_bucket", "cell_first_line", "cell_lines", "cell_stats", "key_cell_begin", "line_cell")
KEY_OUTS = ("key_units", "key_offsets", "key_first_line", "key_lines", "key_stats", "line_key")


def raw_call(gorp, data, offsets, ids, caps, parts, width, max_cells, max_buckets=None, max_keys=64, want=OUTS + KEY_OUTS, poison=0xAB):
    """gx_group_series itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p, numbers = gorp.series_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n = len(offsets) - 1
    max_buckets = max_cells if max_buckets is None else max_buckets
    sizes = {"bucket_number": 8 * (max_buckets + 8), "cell_key": 4 * (max_cells + 8), "cell_bucket": 4 * (max_cells + 8), "cell_first_line": 4 * (max_cells + 8),
             "cell_lines": 8 * (max_cells + 8), "cell_stats": 64 * (max_cells + 8), "key_cell_begin": 8 * (max_keys + 9), "line_cell": 4 * (n + 8),
             "key_units": 4096, "key_offsets": 4 * (max_keys + 9), "key_first_line": 4 * (max_keys + 8), "key_lines": 8 * (max_keys + 8), "key_stats": 64 * (max_keys + 8),
             "line_key": 4 * (n + 8)}
    arrays = {name: np.full(size, poison, np.uint8) for name, size in sizes.items()}
    ptr = lambda name: arrays[name].ctypes.data if name in want and (p.has_values or not name.endswith("_stats")) else None
    keys = N.gx_group_out(ptr("key_units"), 4096, ptr("key_offsets"), ptr("key_first_line"), ptr("key_lines"), ptr("key_stats"), ptr("line_key"), max_keys)
    out = N.gx_series_out(*[ptr(name) for name in OUTS], max_cells, max_buckets)
    totals = N.gx_series_totals()
    rc = N.lib().gx_group_series(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, numbers, 0, width, None, 0, 0,
                                 C.byref(keys), C.byref(out), C.byref(totals), C.byref(o))
    return rc, Gorp._series_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a == poison).all() for a in arrays.values())


def test_capacities_a_full_table_and_the_key_tables_own_overflow():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(33)
    cell = rng.permutation(np.repeat(np.arange(33), 6))                                       # 33 cells: 3 keys x 11 buckets
    data, offsets, ids, caps = batch(names(cell % 3) + [b"k0", b"k1"], (cell // 3).tolist() + [None, b"x"], values=[1] * 200)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 33, max_buckets=11)                   # exactly sufficient
    assert rc == N.GX_OK and (totals["n_cells"], totals["n_buckets"], totals["celled"], totals["number_unset"], totals["not_numbers"]) == (33, 11, 198, 1, 1)
    assert arrays["cell_key"].view(np.uint32)[:33].tolist() == sorted((cell % 3).tolist())[::6] and (arrays["cell_key"][4 * 33:] == 0xAB).all()
    assert arrays["bucket_number"].view(np.int64)[:11].tolist() == list(range(11)) and (arrays["bucket_number"][8 * 11:] == 0xAB).all()
    assert arrays["key_cell_begin"].view(np.uint64)[:4].tolist() == [0, 11, 22, 33] and (arrays["key_cell_begin"][8 * 4:] == 0xAB).all()
    fit = totals
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 32, max_buckets=11)                   # one cell too few: nothing is written
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_cells" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 33, max_buckets=10)                   # one bucket too few
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_buckets" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 33, max_buckets=10, want=tuple(o for o in OUTS + KEY_OUTS if o != "bucket_number"))
    assert rc == N.GX_OK and totals == fit                                                                     # ... binds bucket_number alone
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 33, max_keys=2, want=("key_cell_begin",))
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_keys" in N.last_error()         # key_cell_begin is sized by max_keys
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 32, want=())                          # the size query passes
    assert rc == N.GX_OK and totals == fit and untouched(arrays)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 1, 32, want=("line_cell", "key_cell_begin", "bucket_number"))   # no per-cell array
    assert rc == N.GX_OK and sorted(set(arrays["line_cell"].view(np.uint32)[:200].tolist())) == list(range(33)) + [NONE]
    # the cell table full: 65 cells, 64 slots
    cell = rng.permutation(np.repeat(np.arange(65), 4))
    full = batch(names(cell % 5), (cell // 5).tolist(), values=[1] * 260)
    for want in (OUTS + KEY_OUTS, ()):
        rc, totals, arrays = raw_call(gorp, *full, PV, 1, 32, want=want)
        assert rc == N.GX_E_LIMIT and not totals["cells_exact"] and totals["n_cells"] == 65 and totals["group"]["exact"] and totals["group"]["n_keys"] == 5
        assert untouched(arrays) and "slots" in N.last_error()
    # the key table's own overflow: the series totals are zero
    rc, totals, arrays = raw_call(gorp, *batch(names(np.arange(65)), [1] * 65, values=[1] * 65), PV, 1, 1024, max_keys=32)
    assert rc == N.GX_E_LIMIT and not totals["group"]["exact"] and totals["group"]["n_keys"] == 65 and untouched(arrays)
    assert [totals[name] for name in SERIES_TOTALS] == [0, 0, 0, 0, 0, 0, True, 0, 0]
    # series == NULL: the call is gx_group_lines, the series totals zero with cells_exact
    p, numbers = gorp.series_parts(PV)
    data, offsets, ids, caps = full
    rc, totals = gorp.group_series_device(data.ctypes.data, offsets.ctypes.data, len(ids), ids.ctypes.data, caps.ctypes.data, (p, numbers), 1, max_keys=8, series=False,
                                          device_pointers=False)
    assert rc == N.GX_OK and totals["group"]["n_keys"] == 5 and [totals[name] for name in SERIES_TOTALS] == [0, 0, 0, 0, 0, 0, True, 0, 0]
    # the Python wrapper asks again with what the totals say
    assert check(gorp, *full, PV, 1, max_cells=4)["totals"]["n_cells"] == 65


def test_the_wrapper_when_the_key_table_and_the_cell_capacity_both_fall_short():
    gorp = trivial_handle(1)
    k = np.arange(70)
    # 70 keys over a key table of 64 slots AND 140 cells over tables of 64 slots: the key table's overflow raises both sizes at once
    got = check(gorp, *batch(names(np.concatenate([k, k])), np.concatenate([k, k + 100]).tolist()), P, 1, max_keys=4, max_cells=4)
    assert got["totals"]["n_keys"] == 70 and got["totals"]["n_cells"] == 140 and got["key_cell_begin"].tolist() == list(range(0, 141, 2))


# ---------------------------------------------------------------------------
# 9. every way the batch is read
# ---------------------------------------------------------------------------
def mixed_batch(n=700, seed=5, **kw):
    rng = np.random.default_rng(seed)
    numbers = (np.sort(rng.integers(0, 5000, n)) + rng.integers(-40, 40, n)).tolist()
    values = rng.integers(-500, 900, n).tolist()
    keys = names(rng.integers(0, 6, n))
    for i in rng.integers(0, n, 25):
        numbers[i] = [None, b"-", b"12x"][i % 3]
    for i in rng.integers(0, n, 25):
        values[i] = [None, b"", b"1e3"][i % 3]
    for i in rng.integers(0, n, 15):
        keys[i] = [None, b""][i % 2]
    ids = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n))
    return batch(keys, numbers, values, lengths=rng.integers(0, 30, n), ids=ids, **kw)


TWO_PARTS = [(0, 0, 1, 2), (1, 0, 1, 2)]


@pytest.mark.parametrize("rows", [np.uint16, np.uint8])
def test_compact_result_rows(rows):
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch()
    got = check(gorp, data, offsets, pack(ids, caps, rows), None, TWO_PARTS, 100, origin=37)
    assert got["totals"]["n_cells"] > 100 and got["totals"]["number_unset"] > 0 and got["totals"]["not_numbers"] > 0 and got["totals"]["unset"] > 0


def test_offsets64_utf16_utf8_bytes_and_where_terms():
    gorp = trivial_handle(2)
    base = check(gorp, *mixed_batch(), TWO_PARTS, 100)
    for kw, utf8 in ((dict(offsets_dtype=np.uint64), None), (dict(dtype=np.uint16), None), (dict(dtype=np.uint16, offsets_dtype=np.uint64), None), ({}, "bytes")):
        got = check(gorp, *mixed_batch(**kw), TWO_PARTS, 100, utf8=utf8)
        assert {k: got["totals"][k] for k in SERIES_TOTALS} == {k: base["totals"][k] for k in SERIES_TOTALS} and got["cell_stats"] == base["cell_stats"]
        assert all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)
    got = check(gorp, *mixed_batch(), TWO_PARTS, 100, where=[(0, 2, ">=", 500), (1, 2, "<", 0)])
    assert 0 < got["totals"]["lines"] < 300 and got["totals"]["n_cells"] > 10


def test_number_formats_iso8601_beside_a_decimal_value():
    gorp = trivial_handle(1, tag="iso")
    gorp.set_number_format(0, 1, "iso8601", 3)
    gorp.set_number_format(0, 2, "decimal", 2)
    stamps = [b"2026-01-03T00:00:01.123Z", b"2026-01-03T00:00:59.999Z", b"2026-01-03T00:01:00.000Z", b"2026-01-02T23:59:59.999Z", b"2026-01-03T01:00:00+01:00",
              b"yesterday", None, b"2026-01-03T00:01:30Z"]
    keys = [b"GET", b"PUT", b"GET", b"GET", b"PUT", b"GET", b"PUT", b"GET"]
    values = [b"0.25", b"1", b"-1.00", b"2.50", b"x", b"1", b"1", b"0.5"]
    formats = {(0, 1): ("iso8601", 3), (0, 2): ("decimal", 2)}
    got = check(gorp, *batch(keys, stamps, values=values), PV, 60_000, origin="2026-01-03T00:00:00Z", formats=formats)
    assert got["bucket_number"].tolist() == [-1, 0, 1] and got["cell_key"].tolist() == [0, 0, 0, 1] and got["cell_bucket"].tolist() == [0, 1, 2, 1]
    assert [s["sum"] for s in got["cell_stats"]] == [250, 25, -50, 100] and got["totals"]["not_numbers"] == 1 and got["totals"]["number_unset"] == 1
    assert got["cell_stats"][2]["numbers"] == 2 and got["cell_stats"][3]["not_numbers"] == 1 and got["cell_stats"][3]["numbers"] == 1


@pytest.fixture
def new_stream():
    """A stream of the test's own, created and destroyed here, not drawn from torch's pool."""
    import torch
    rt = N._load_hip_runtime()
    rt.hipStreamCreateWithFlags.argtypes, rt.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
    made = []

    def make():
        s = C.c_void_p()
        assert rt.hipStreamCreateWithFlags(C.byref(s), 1) == 0     # hipStreamNonBlocking, as torch's own are
        made.append(s)
        return torch.cuda.ExternalStream(s.value)
    yield make
    torch.cuda.synchronize()
    for s in made:
        assert rt.hipStreamDestroy(s) == 0


def test_device_pointers_on_a_side_stream_the_size_query_and_two_runs_are_the_same_bits(new_stream):
    import torch
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch(n=5000, seed=9)
    host = check(gorp, data, offsets, ids, caps, TWO_PARTS, 100, max_cells=1024)
    t = host["totals"]
    c, b, k, n = t["n_cells"], t["n_buckets"], t["n_keys"], len(ids)
    dev = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    d_data, d_off, d_ids, d_caps = dev(data), dev(offsets), dev(ids), dev(caps)
    stream = new_stream()
    torch.cuda.synchronize()
    args = (d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), TWO_PARTS, 100)
    with torch.cuda.stream(stream):
        rc, totals = gorp.group_series_device(*args, max_keys=8, max_cells=c, stream=stream.cuda_stream)       # the size query: every output NULL
    assert rc == N.GX_OK and totals == t
    runs = []
    for _ in range(2):
        mk = lambda count, dtype: torch.full((count + 4,), 0x5A, dtype=dtype, device="cuda")
        out = {"bucket_number": mk(b, torch.int64), "cell_key": mk(c, torch.int32), "cell_bucket": mk(c, torch.int32), "cell_first_line": mk(c, torch.int32),
               "cell_lines": mk(c, torch.int64), "cell_stats": mk(8 * c, torch.int64), "key_cell_begin": mk(k + 1, torch.int64), "line_cell": mk(n, torch.int32),
               "line_key": mk(n, torch.int32), "key_lines": mk(k, torch.int64)}
        with torch.cuda.stream(stream):
            rc, totals = gorp.group_series_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                                  max_cells=c, max_buckets=b, stream=stream.cuda_stream,
                                                  **{name + "_ptr": out[name].data_ptr() for name in OUTS})
        stream.synchronize()                                                                   # the outputs are read after a stream wait
        assert rc == N.GX_OK and totals == t
        runs.append({name: a.cpu().numpy() for name, a in out.items()})
    x, y = runs
    assert all(x[name].tobytes() == y[name].tobytes() for name in x)
    for name, dtype in SERIES_FIELDS:
        m = len(host[name])
        assert x[name][:m].view(dtype).tolist() == host[name].tolist() and (x[name][m:] == 0x5A).all(), name
    assert x["line_key"][:n].view(np.uint32).tolist() == host["line_key"].tolist() and x["key_lines"][:k].tolist() == host["lines"].tolist()
    stats = x["cell_stats"][:8 * c].reshape(c, 8)
    assert (x["cell_stats"][8 * c:] == 0x5A).all()
    for j, s in enumerate(host["cell_stats"]):
        assert stats[j, :4].tolist() == [s["lines"], s["numbers"], s["unset"], s["not_numbers"]]
        assert s["numbers"] == 0 or (int(stats[j, 4]), int(stats[j, 5])) == (s["min"], s["max"])
        assert (int(stats[j, 7]) << 64) + (int(stats[j, 6]) & (2 ** 64 - 1)) == s["sum"]


# ---------------------------------------------------------------------------
# 10. end to end: the syslog workload, extracted on the device, host x minute, and the same from raw text
# ---------------------------------------------------------------------------
def test_syslog_host_by_minute_end_to_end_and_from_raw_text():
    rules, meta = W.syslog_definition(4)
    gorp = Gorp.construct(rules)
    data, offsets, _ = W.syslog_lines(meta, 1500, seed=11)
    data, offsets = np.asarray(data, np.uint8), np.asarray(offsets, np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids >= 0).sum() > 1400 and (ids < 0).sum() > 3
    for k in range(4):
        gorp.set_number_format(k, "ts", "iso8601", 3)
    parts = [("rule%d" % k, "host", "ts") for k in range(3)] + [("rule3", "host", "ts", "pid")]
    formats = {(k, gorp._extraction_and_group(k, "ts")[1]): ("iso8601", 3) for k in range(4)}
    origin = "2026-01-01T00:00:00Z"
    got = check(gorp, data, offsets, ids, caps, parts, 60_000, origin=origin, formats=formats, max_cells=64)
    t = got["totals"]
    assert t["n_cells"] > 64 and t["celled"] > 1400 and t["n_keys"] > 1 and t["n_buckets"] > 1                  # (more than max_cells: asked twice)
    assert gorp._series_origin(gorp.series_parts(parts), origin) == parse_number("iso8601", 3, origin)
    # the whole-file form: raw text in, the same keys and cells out, counts and n_lines as text_group_lines gives them
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))]
    raw = b"\n".join(lines) + b"\n"
    text, counts, n_lines = gorp.text_group_series(raw, parts, 60_000, origin=origin)
    keys, kcounts, kn = gorp.text_group_lines(raw, gorp.series_parts(parts)[0])
    assert n_lines == kn == len(ids) and counts.tolist() == kcounts.tolist() and counts[:4].tolist() == [int((ids == k).sum()) for k in range(4)]
    assert text["totals"] == got["totals"] and text["cell_stats"] == got["cell_stats"] and text["keys"] == got["keys"] == keys["keys"]
    assert all(text[f].tobytes() == got[f].tobytes() for f in FIELDS + KEY_FIELDS) and text["totals"]["group"] == keys["totals"]


# ---------------------------------------------------------------------------
# 11. one large shape
# ---------------------------------------------------------------------------
def test_two_hundred_thousand_lines_against_numpy():
    gorp = trivial_handle(1)
    n = 200_000
    key, v, matched = draw(n, seed=20)
    data, offsets, ids, caps = digits_batch(key, v, matched)
    for origin, width in ((0, 60_000), (123_456, 50_000)):
        want = np_series(key, v, matched, origin, width)
        got = gorp.group_series(data, offsets, ids, caps, P, width, origin, max_cells=4096)
        t = got["totals"]
        assert t["n_cells"] == len(want["cell_key"]) and t["celled"] == t["keyed"] == t["lines"] == int(matched.sum()) and t["cells_exact"] and t["n_keys"] == 6
        assert (t["first_bucket"], t["last_bucket"], t["n_buckets"]) == (int(want["bucket_number"][0]), int(want["bucket_number"][-1]), len(want["bucket_number"]))
        for name, dtype in SERIES_FIELDS:
            assert got[name].dtype == want[name].dtype == dtype and np.array_equal(got[name], want[name]), name
        keys = gorp.group_lines(data, offsets, ids, caps, [(0, 0)])
        assert got["totals"]["group"] == keys["totals"] and all(got[f].tobytes() == keys[f].tobytes() for f in KEY_FIELDS)
    assert 300 < t["n_buckets"] < 1000 and t["n_cells"] > 1500
