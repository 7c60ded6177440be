"""GPU tests of gx_group_windows / gx_text_group_windows: for every entry of a key -- its lines ordered by a captured time -- the key's
lines within `window` before it, the trips at which that count reaches a threshold from below, every key's peak, the windows' sums.

Expected values come from tests/windows_oracle.py -- per key a list sorted by (time, line) and the caller's deque loop over Python's
integers -- and everything is compared bit for bit.  In every case the key outputs and totals["group"] are compared byte for byte with
gx_group_lines' on the same arguments, and the case runs once more under GX_BUCKET_ALL_DIGITS, under GX_GROUP_WEAK_HASH and under both,
and must give the same bytes.  Batches are fabricated as tests/test_gpu_sessions.py fabricates them.  The large shape is compared with
a numpy restatement (searchsorted per key on the order-preserving words), which tests/test_windows_host.py compares with the oracle on
smaller draws of the same generator.  The shapes are the smallest at which a pass can still go wrong: the edges of a wave (64), of a
workgroup (256), of the sort's block and the scan's tile (2 048); key runs at every distance from a power of two for the gallop."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp
from number_oracle import KINDS
from where_oracle import decode_terms, unpack
from windows_oracle import INT64_MAX, INT64_MIN, NONE, WINDOW_FIELDS, WINDOW_TOTALS, batch, decode_parts, draw, group_windows, np_windows, same, wide_batch

pytestmark = pytest.mark.gpu

BLOCK = 2048              # gx_scan.hpp's tile and the sort's block (BKT_BLOCK)
P = [(0, 0, 1)]           # extraction 0: group 0 the key, group 1 the time
PV = [(0, 0, 1, 2)]       # ... and group 2 measured
KEY_FIELDS = ("key_units", "key_offsets", "first_line", "lines", "line_key")
FIELDS = tuple(name for name, _ in WINDOW_FIELDS)


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, window, threshold=0, where=None, utf8=None, formats=None, hooks=True, **kw):
    """group_windows against the restatement, every field; the keys against group_lines on the same arguments, byte for byte; then under
    the test hooks, the same bytes.  Returns what the call returned."""
    both = gorp.series_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    fm = {key: (KINDS[kind], scale) for key, (kind, scale) in (formats or {}).items()}
    want = group_windows(data, offsets, ids, caps, decode_parts(both), gorp._windows_window(both, window), threshold, decode_terms(terms), gorp.num_extractions, fm)
    got = gorp.group_windows(data, offsets, ids, caps, both, window, threshold, where=terms, utf8=utf8, **kw)
    same(got, want)
    t = got["totals"]
    assert t["keyed"] == t["entries"] + t["number_unset"] + t["not_numbers"]
    keys = gorp.group_lines(data, offsets, ids, caps, both[0], where=terms, utf8=utf8, max_keys=kw.get("max_keys"))
    assert t["group"] == keys["totals"] and got["stats"] == keys["stats"] and got["keys"] == keys["keys"]
    for name in KEY_FIELDS:
        assert got[name].dtype == keys[name].dtype and got[name].tobytes() == keys[name].tobytes(), name
    for hook in ([dict(all_digits=True), dict(weak_hash=True), dict(weak_hash=True, all_digits=True)] if hooks else []):
        if hook.get("weak_hash") and t["n_keys"] > 4096:
            continue
        again = gorp.group_windows(data, offsets, ids, caps, both, window, threshold, where=terms, utf8=utf8, **dict(kw, **hook))
        assert again["totals"] == got["totals"] and again["entry_window_sum"] == got["entry_window_sum"] and again["stats"] == got["stats"], hook
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
# 1. what a window and a trip are
# ---------------------------------------------------------------------------
def test_seven_lines_two_keys_a_burst_over_an_interval_edge_trips_once_and_thinned_never():
    gorp = trivial_handle(1)
    # u1's burst 58, 59, 61 straddles the edge at 60 of a series of width 60: 2 + 1 there, three within 10 here
    keys = [b"u1", b"u2", b"u1", b"u1", b"u2", b"u1", b"u2"]
    got = check(gorp, *batch(keys, [58, 10, 59, 61, 70, 200, 130], values=[1, 2, 3, 4, 5, 6, 7]), PV, 10, 3)
    assert got["keys"] == [b"u1", b"u2"] and got["entry_line"].tolist() == [0, 2, 3, 5, 1, 4, 6] and got["entry_key"].tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert got["entry_time"].tolist() == [58, 59, 61, 200, 10, 70, 130] and got["entry_window_lines"].tolist() == [1, 2, 3, 1, 1, 1, 1]
    assert got["line_window_lines"].tolist() == [1, 1, 2, 3, 1, 1, 1] and got["key_entry_begin"].tolist() == [0, 4, 7]
    assert (got["trip_key"].tolist(), got["trip_line"].tolist(), got["trip_time"].tolist(), got["trip_entry"].tolist()) == ([0], [3], [61], [2])
    assert got["key_trip_begin"].tolist() == [0, 1, 1] and got["key_peak_lines"].tolist() == [3, 1] and got["key_peak_line"].tolist() == [3, 1]
    assert [s["sum"] for s in got["entry_window_sum"]] == [1, 4, 8, 6, 2, 5, 7] and [s["numbers"] for s in got["entry_window_sum"]] == [1, 2, 3, 1, 1, 1, 1]
    t = got["totals"]
    assert [t[name] for name in WINDOW_TOTALS] == [7, 0, 0, 1, 1, 3, 3, 0, 10, 200]
    got = check(gorp, *batch(keys, [58, 10, 48, 69, 70, 200, 130]), P, 10, 3)                                 # the burst thinned: 48, 58, 69
    assert got["totals"]["n_trips"] == 0 and got["totals"]["tripped_keys"] == 0 and len(got["trip_key"]) == 0 and got["key_trip_begin"].tolist() == [0, 0, 0]
    assert got["entry_window_lines"].tolist() == [1, 2, 1, 1, 1, 1, 1] and got["totals"]["peak_lines"] == 2


# ---------------------------------------------------------------------------
# 2. block edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_entries_at_the_edges_of_a_wave_a_workgroup_a_sort_block_and_a_scan_tile(m):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(m)
    order = rng.permutation(m)                                                                   # one key, times 1 apart, in no order
    keys, times = names([0] * m), order.tolist()
    for i in range(0, m, 97):                                                                    # a few lines that are no entries between them
        keys.insert(i, b"k0")
        times.insert(i, [None, b"x"][i % 2])
    got = check(gorp, *batch(keys, times, values=list(range(len(keys)))), PV, 100, 101)
    assert got["totals"]["entries"] == m and got["entry_window_lines"].tolist() == [min(e, 100) + 1 for e in range(m)]
    assert got["totals"]["n_trips"] == (1 if m > 100 else 0) and got["trip_entry"].tolist() == ([100] if m > 100 else [])


def test_one_key_of_one_time_and_every_entry_its_own_key():
    gorp = trivial_handle(1)
    n = 5000
    got = check(gorp, *batch(names([0] * n), [7] * n, values=list(range(n))), PV, 0, 4097)                     # the gallop reaches the run's start
    assert got["entry_window_lines"].tolist() == list(range(1, n + 1)) and got["entry_line"].tolist() == list(range(n))
    assert got["totals"]["peak_lines"] == n and got["totals"]["peak_line"] == n - 1 and got["trip_entry"].tolist() == [4096]
    assert got["entry_window_sum"][-1] == {"numbers": n, "sum": n * (n - 1) // 2}
    got = check(gorp, *batch(names(np.arange(n)), [7] * n), P, INT64_MAX, 1, max_keys=n, hooks=False)         # every gallop stops at once
    assert set(got["entry_window_lines"].tolist()) == {1} and got["totals"]["n_trips"] == got["totals"]["tripped_keys"] == n
    assert got["key_entry_begin"].tolist() == list(range(n + 1)) == got["key_trip_begin"].tolist() and (got["totals"]["peak_line"], got["totals"]["peak_key"]) == (0, 0)
    got = check(gorp, *batch(names(np.arange(300)), [7] * 300), P, 5, 1)                                       # ... and under the hooks
    assert got["trip_key"].tolist() == list(range(300))


def test_key_runs_at_every_distance_from_a_power_of_two():
    gorp = trivial_handle(1)
    runs = [1, 2, 3, 64, 65, 1023]
    k = np.concatenate([np.full(c, j) for j, c in enumerate(runs)])
    t = np.concatenate([np.arange(c) for c in runs])                                             # window larger than any span: lo is the key's first entry
    got = check(gorp, *batch(names(k), t.tolist()), P, 10 ** 6, 64)
    assert got["entry_window_lines"].tolist() == [e + 1 for c in runs for e in range(c)] and got["key_peak_lines"].tolist() == runs
    assert got["trip_key"].tolist() == [3, 4, 5] and got["key_entry_begin"].tolist() == np.concatenate([[0], np.cumsum(runs)]).tolist()
    rng = np.random.default_rng(4)
    order = rng.permutation(len(k))                                                              # the same in no order, the keys' numbers another way round
    got = check(gorp, *batch(names(k[order]), t[order].tolist()), P, 10 ** 6, 3)
    assert sorted(got["key_peak_lines"].tolist()) == runs and got["totals"]["tripped_keys"] == 4 == got["totals"]["n_trips"]


# ---------------------------------------------------------------------------
# 3. order
# ---------------------------------------------------------------------------
def test_descending_and_shuffled_times_ties_and_two_keys_interleaved():
    gorp = trivial_handle(1)
    got = check(gorp, *batch(names([0] * 300), list(range(3000, 0, -10))), P, 25, 3)                           # descending: reversed, three per window
    assert got["entry_line"].tolist() == list(range(299, -1, -1)) and got["entry_window_lines"].tolist() == [1, 2] + [3] * 298 and got["trip_entry"].tolist() == [2]
    # ties in time inside a key: the order goes by input line, and a tie's later line is not in the earlier one's window
    got = check(gorp, *batch(names([0, 1, 0, 0, 1, 0]), [50, 50, 50, 40, 50, 50]), P, 0, 2)
    assert got["entry_line"].tolist() == [3, 0, 2, 5, 1, 4] and got["entry_window_lines"].tolist() == [1, 1, 2, 3, 1, 2]
    assert got["trip_line"].tolist() == [2, 4] and got["line_window_lines"].tolist() == [1, 1, 2, 1, 2, 3]
    # two keys interleaved line by line: A every 10, B between them -- A's window must not see B's entries
    a, b = np.arange(200) * 10, np.arange(200) * 10 + 5
    keys = [x for pair in zip(names([0] * 200), names([1] * 200)) for x in pair]
    times = [int(x) for pair in zip(a, b) for x in pair]
    got = check(gorp, *batch(keys, times), P, 10, 2)
    assert got["entry_window_lines"].tolist() == ([1] + [2] * 199) * 2 and got["trip_entry"].tolist() == [1, 201]
    rng = np.random.default_rng(3)
    k, t = rng.integers(0, 9, 3000), rng.integers(-40_000, 40_000, 3000)
    got = check(gorp, *batch(names(k), t.tolist(), values=rng.integers(-50, 50, 3000).tolist()), PV, 400, 5)
    assert (np.diff(got["trip_key"].astype(np.int64)) >= 0).all() and got["totals"]["n_trips"] > 50 and got["totals"]["n_trips"] > got["totals"]["tripped_keys"] == 9


# ---------------------------------------------------------------------------
# 4. arithmetic
# ---------------------------------------------------------------------------
def test_the_corners_of_int64_window_zero_and_a_difference_of_exactly_the_window():
    gorp = trivial_handle(1)
    got = check(gorp, *batch(names([0] * 4), [INT64_MAX, 0, INT64_MIN, -1]), P, INT64_MAX, 2)
    assert got["entry_time"].tolist() == [INT64_MIN, -1, 0, INT64_MAX] and got["entry_window_lines"].tolist() == [1, 2, 2, 2]     # INT64_MIN is in -1's alone
    assert (got["totals"]["first_time"], got["totals"]["last_time"]) == (INT64_MIN, INT64_MAX) and got["trip_entry"].tolist() == [1]
    got = check(gorp, *batch(names([0] * 2), [INT64_MAX, INT64_MIN]), P, INT64_MAX, 2)
    assert got["entry_window_lines"].tolist() == [1, 1] and got["totals"]["n_trips"] == 0
    got = check(gorp, *batch(names([0] * 6), [-100, -70, -39, -9, 21, 52]), P, 30, 2)                          # 30, 31, 30, 30, 31 apart
    assert got["entry_window_lines"].tolist() == [1, 2, 1, 2, 2, 1] and got["trip_time"].tolist() == [-70, -9]
    got = check(gorp, *batch(names([0] * 6), [-100, -70, -39, -9, 21, 52]), P, 29, 2)
    assert got["entry_window_lines"].tolist() == [1] * 6
    got = check(gorp, *batch(names([0] * 5), [5, 6, 6, 8, 6]), P, 0, 3)                                        # window 0: the same time up to e
    assert got["entry_window_lines"].tolist() == [1, 1, 2, 3, 1] and got["trip_line"].tolist() == [4]


def test_thresholds_one_retrips_none_and_peak_ties():
    gorp = trivial_handle(1)
    keys = names([0, 1, 0, 2, 1, 0]) + [b"k3"]
    got = check(gorp, *batch(keys, [5, 5, 6, 9, 7, 7, None]), P, 100, 1)                                       # threshold 1: the keys with entries
    assert got["trip_key"].tolist() == [0, 1, 2] and got["trip_entry"].tolist() == [0, 3, 5] and got["totals"]["tripped_keys"] == 3 and got["totals"]["n_keys"] == 4
    assert got["key_trip_begin"].tolist() == [0, 1, 2, 3, 3] and got["key_peak_lines"].tolist() == [3, 2, 1, 0] and got["key_peak_line"].tolist() == [5, 4, 3, NONE]
    t = [0, 1, 2, 3, 50, 51, 52, 53, 54, 200, 201, 202]                                                       # trips, falls below, trips again, and again
    got = check(gorp, *batch(names([0] * 12), t), P, 10, 3)
    assert got["trip_time"].tolist() == [2, 52, 202] and got["totals"]["n_trips"] == 3 and got["totals"]["tripped_keys"] == 1
    assert got["key_peak_lines"].tolist() == [5] and got["key_peak_line"].tolist() == [8]
    got = check(gorp, *batch(names([0] * 12), t), P, 10, 6)                                                   # above every count: no trips, trip outputs legal
    assert got["totals"]["n_trips"] == 0 and len(got["trip_entry"]) == 0 and got["key_trip_begin"].tolist() == [0, 0]
    got = check(gorp, *batch(names([0] * 12), t), P, 10, 2 ** 32 - 1)
    assert got["totals"]["n_trips"] == 0
    got = check(gorp, *batch(names([0] * 12), t), P, 10, 0)                                                   # threshold 0: no trips, no trip outputs passed
    assert got["totals"]["n_trips"] == 0 and len(got["trip_key"]) == 0 and got["entry_window_lines"].tolist() == [1, 2, 3, 4, 1, 2, 3, 4, 5, 1, 2, 3]
    # peak ties within a key (4 attained at 3 and again at 13) and across keys (key 1 attains 4 too, later in the order)
    k = [0] * 8 + [1] * 4
    t = [0, 1, 2, 3, 10, 11, 12, 13] + [0, 1, 2, 3]
    got = check(gorp, *batch(names(k), t), P, 5, 4)
    assert got["key_peak_lines"].tolist() == [4, 4] and got["key_peak_line"].tolist() == [3, 11]
    assert (got["totals"]["peak_lines"], got["totals"]["peak_line"], got["totals"]["peak_key"]) == (4, 3, 0) and got["trip_line"].tolist() == [3, 7, 11]
    got = check(gorp, *batch(names(k[::-1]), t[::-1]), P, 5, 4)                                               # the lines reversed: key 1 comes first
    assert got["keys"] == [b"k1", b"k0"] and (got["totals"]["peak_lines"], got["totals"]["peak_line"], got["totals"]["peak_key"]) == (4, 0, 0)
    assert got["key_peak_line"].tolist() == [0, 8]


def test_128_bit_window_sums():
    gorp = trivial_handle(1)
    big = [INT64_MAX, INT64_MAX, INT64_MIN, INT64_MIN, INT64_MIN, INT64_MAX - 1, 5, None, b"x", -7]
    got = check(gorp, *batch(names([0] * 10), list(range(0, 100, 10)), values=big), PV, 20, 2)
    sums = [s["sum"] for s in got["entry_window_sum"]]
    assert sums[1] == 2 * INT64_MAX and sums[2] == 2 * INT64_MAX + INT64_MIN and sums[4] == 3 * INT64_MIN and sums[3] == INT64_MAX + 2 * INT64_MIN
    assert [s["numbers"] for s in got["entry_window_sum"]] == [1, 2, 3, 3, 3, 3, 3, 2, 1, 1]
    got = check(gorp, *batch(names([0] * 4), [0, 100, 200, 300], values=[None, b"q", None, 4]), PV, 10, 0)     # windows that hold no number
    assert got["entry_window_sum"] == [{"numbers": 0, "sum": 0}] * 3 + [{"numbers": 1, "sum": 4}]
    rng = np.random.default_rng(8)
    n = 3 * BLOCK + 5                                                                             # sums that leave int64 across the scans' tiles
    values = rng.choice([INT64_MAX, INT64_MIN, INT64_MAX - 3, -1, 0, 17], n).tolist()
    got = check(gorp, *batch(names(rng.integers(0, 2, n)), rng.integers(0, 4000, n).tolist(), values=values), PV, 700, 0, hooks=False)
    assert any(not INT64_MIN <= s["sum"] <= INT64_MAX for s in got["entry_window_sum"]) and got["totals"]["peak_lines"] > 256


# ---------------------------------------------------------------------------
# 5. classes, parts, terms
# ---------------------------------------------------------------------------
def test_each_class_of_keyed_line_adds_up_and_a_part_without_a_number():
    gorp = trivial_handle(2)
    keys = [b"x", b"x", b"y", b"x", None, b"y", b"y", b"z", b"x", b"y"]
    times = [5, -2 ** 63, None, b"12x", 7, b"", 6, 8, 5, 5]
    ids = [0, 0, 0, 0, 0, 0, 1, 1, -1, 0]
    data, offsets, ids, caps = batch(keys, times, values=[1, 2, 3, 4, 5, 6, 7, None, 9, b"q"], lengths=[9] * 10, ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, 1, 2)], 1, 2)
    t = got["totals"]
    assert (t["lines"], t["keyed"], t["unset"], t["entries"], t["number_unset"], t["not_numbers"]) == (9, 8, 1, 5, 1, 2)
    assert got["keys"] == [b"x", b"y", b"z"] and got["entry_line"].tolist() == [1, 0, 9, 6, 7] and got["line_window_lines"].tolist() == [1, 1, 0, 0, 0, 0, 2, 1, 0, 1]
    # number_groups = -1 for one of two parts: extraction 1's lines have a key and no time; two extractions share the keys
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, None, 2)], 1, 1)
    t = got["totals"]
    assert (t["keyed"], t["entries"], t["number_unset"]) == (8, 3, 3) and got["key_entry_begin"].tolist() == [0, 2, 3, 3] and got["key_peak_lines"].tolist() == [1, 1, 0]
    # no part at all, and no line at all: all zeros, the bounds' one entry, every line's 0
    got = check(gorp, data, offsets, ids, caps, [], 1, 2)
    assert got["totals"]["entries"] == 0 and got["key_entry_begin"].tolist() == [0] == got["key_trip_begin"].tolist() and set(got["line_window_lines"].tolist()) == {0}
    got = check(gorp, *batch([], []), P, 1, 2)
    assert got["totals"]["entries"] == 0 and len(got["line_window_lines"]) == 0 and got["key_entry_begin"].tolist() == [0] == got["key_trip_begin"].tolist()
    assert got["entry_window_sum"] is None and len(got["entry_line"]) == 0 and len(got["trip_key"]) == 0 and got["keys"] == []
    got = check(gorp, *batch([b"a", b"b"], [None, b"x"]), P, 1, 2)                              # keyed lines, none of them an entry
    assert got["key_entry_begin"].tolist() == [0, 0, 0] == got["key_trip_begin"].tolist() and got["line_window_lines"].tolist() == [0, 0]
    assert got["key_peak_lines"].tolist() == [0, 0] and got["key_peak_line"].tolist() == [NONE, NONE]
    assert [got["totals"][name] for name in WINDOW_TOTALS] == [0, 1, 1, 0, 0, 0, NONE, NONE, 0, 0]


def mixed_batch(n=700, seed=5, **kw):
    rng = np.random.default_rng(seed)
    times = (np.sort(rng.integers(0, 5000, n)) + rng.integers(-40, 40, n)).tolist()
    values = rng.integers(-500, 900, n).tolist()
    keys = names(rng.integers(0, 6, n))
    for i in rng.integers(0, n, 25):
        times[i] = [None, b"-", b"12x"][i % 3]
    for i in rng.integers(0, n, 25):
        values[i] = [None, b"", b"1e3"][i % 3]
    for i in rng.integers(0, n, 15):
        keys[i] = [None, b""][i % 2]
    ids = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n))
    return batch(keys, times, values, lengths=rng.integers(0, 30, n), ids=ids, **kw)


TWO_PARTS = [(0, 0, 1, 2), (1, 0, 1, 2)]


# ---------------------------------------------------------------------------
# 6. every way the batch is read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [np.uint16, np.uint8])
def test_compact_result_rows(rows):
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch()
    got = check(gorp, data, offsets, pack(ids, caps, rows), None, TWO_PARTS, 60, 4)
    assert got["totals"]["n_trips"] > 5 and got["totals"]["number_unset"] > 0 and got["totals"]["not_numbers"] > 0 and got["totals"]["unset"] > 0


def test_offsets64_utf16_utf8_bytes_and_where_terms():
    gorp = trivial_handle(2)
    base = check(gorp, *mixed_batch(), TWO_PARTS, 60, 4)
    for kw, utf8 in ((dict(offsets_dtype=np.uint64), None), (dict(dtype=np.uint16), None), (dict(dtype=np.uint16, offsets_dtype=np.uint64), None), ({}, "bytes")):
        got = check(gorp, *mixed_batch(**kw), TWO_PARTS, 60, 4, utf8=utf8)
        assert {k: got["totals"][k] for k in WINDOW_TOTALS} == {k: base["totals"][k] for k in WINDOW_TOTALS} and got["entry_window_sum"] == base["entry_window_sum"]
        assert all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)
    got = check(gorp, *mixed_batch(), TWO_PARTS, 60, 2, where=[(0, 2, ">=", 500), (1, 2, "<", 0)])
    assert 0 < got["totals"]["lines"] < 300 and got["totals"]["n_trips"] > 3


def test_number_formats_iso8601_with_the_window_in_milliseconds():
    gorp = trivial_handle(1, tag="iso")
    gorp.set_number_format(0, 1, "iso8601", 3)
    gorp.set_number_format(0, 2, "decimal", 2)
    stamps = [b"2026-01-03T00:00:01.123Z", b"2026-01-03T00:00:31.123Z", b"2026-01-03T00:01:01.124Z", b"2026-01-02T23:59:59.999Z", b"2026-01-03T01:00:00+01:00",
              b"yesterday", None, b"2026-01-03T00:01:30Z"]
    keys = [b"GET", b"PUT", b"GET", b"GET", b"PUT", b"GET", b"PUT", b"GET"]
    values = [b"0.25", b"1", b"-1.00", b"2.50", b"x", b"1", b"1", b"0.5"]
    formats = {(0, 1): ("iso8601", 3), (0, 2): ("decimal", 2)}
    got = check(gorp, *batch(keys, stamps, values=values), PV, 60_000, 2, formats=formats)              # GET: 23:59:59.999, 00:00:01.123, 00:01:01.124, 00:01:30
    assert got["entry_line"].tolist() == [3, 0, 2, 7, 4, 1] and got["entry_window_lines"].tolist() == [1, 2, 1, 2, 1, 2] and got["trip_line"].tolist() == [0, 7, 1]
    assert [s["sum"] for s in got["entry_window_sum"]] == [250, 275, -100, -50, 0, 100] and got["totals"]["not_numbers"] == 1 and got["totals"]["number_unset"] == 1
    got = check(gorp, *batch(keys, stamps, values=values), PV, 60_001, 3, formats=formats)              # one millisecond more: 00:00:01.123 is in 00:01:01.124's
    assert got["entry_window_lines"].tolist() == [1, 2, 2, 2, 1, 2] and got["totals"]["n_trips"] == 0
    got = check(gorp, *batch(keys, stamps, values=values), PV, 90_001, 4, formats=formats)                 # 23:59:59.999 is in 00:01:30's
    assert got["entry_window_lines"].tolist() == [1, 2, 3, 4, 1, 2] and got["trip_line"].tolist() == [7]


# ---------------------------------------------------------------------------
# 7. the calling forms
# ---------------------------------------------------------------------------
OUTS = Gorp.WINDOW_OUTS
KEY_OUTS = ("key_units", "key_offsets", "key_first_line", "key_lines", "key_stats", "line_key")
PER_ENTRY = {"entry_line": 4, "entry_key": 4, "entry_time": 8, "entry_window_lines": 4, "entry_window_sum": 32}
PER_TRIP = {"trip_key": 4, "trip_line": 4, "trip_time": 8, "trip_entry": 4}
PER_KEY = {"key_entry_begin": 8, "key_peak_lines": 4, "key_peak_line": 4, "key_trip_begin": 8}


def raw_call(gorp, data, offsets, ids, caps, parts, window, threshold, max_entries, max_trips, max_keys=64, want=OUTS + KEY_OUTS, poison=0xAB, windows=True):
    """gx_group_windows itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p, numbers = gorp.series_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n = len(offsets) - 1
    sizes = {name: w * (max_entries + 8) for name, w in PER_ENTRY.items()}
    sizes.update({name: w * (max_trips + 8) for name, w in PER_TRIP.items()})
    sizes.update({name: w * (max_keys + 9) for name, w in PER_KEY.items()})
    sizes.update({"line_window_lines": 4 * (n + 8), "key_units": 4096, "key_offsets": 4 * (max_keys + 9), "key_first_line": 4 * (max_keys + 8),
                  "key_lines": 8 * (max_keys + 8), "key_stats": 64 * (max_keys + 8), "line_key": 4 * (n + 8)})
    arrays = {name: np.full(size, poison, np.uint8) for name, size in sizes.items()}
    ptr = lambda name: arrays[name].ctypes.data if name in want and (p.has_values or name not in ("key_stats", "entry_window_sum")) else None
    keys = N.gx_group_out(ptr("key_units"), 4096, ptr("key_offsets"), ptr("key_first_line"), ptr("key_lines"), ptr("key_stats"), ptr("line_key"), max_keys)
    out = N.gx_windows_out(*[ptr(name) for name in OUTS], max_entries, max_trips)
    totals = N.gx_windows_totals()
    rc = N.lib().gx_group_windows(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, numbers, window, threshold, None,
                                  0, 0, C.byref(keys), C.byref(out) if windows else None, C.byref(totals), C.byref(o))
    return rc, Gorp._windows_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a == poison).all() for a in arrays.values())


def test_capacities_poisoned_outputs_the_size_query_and_windows_null():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(33)
    cell = rng.permutation(np.repeat(np.arange(33), 6))                                       # 3 keys x 11 bursts of 6 entries of one time, 100 apart
    data, offsets, ids, caps = batch(names(cell % 3) + [b"k0", b"k1"], (cell // 3 * 100).tolist() + [None, b"x"], values=[1] * 200)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 198, 33)                          # exactly sufficient
    assert rc == N.GX_OK and [totals[name] for name in WINDOW_TOTALS[:6]] == [198, 1, 1, 33, 3, 6]
    assert arrays["trip_key"].view(np.uint32)[:33].tolist() == [0] * 11 + [1] * 11 + [2] * 11 and (arrays["trip_key"][4 * 33:] == 0xAB).all()
    assert arrays["trip_time"].view(np.int64)[:11].tolist() == list(range(0, 1100, 100)) and (arrays["trip_time"][8 * 33:] == 0xAB).all()
    assert arrays["trip_entry"].view(np.uint32)[:33].tolist() == list(range(3, 198, 6)) and (arrays["trip_line"][4 * 33:] == 0xAB).all()
    assert arrays["key_entry_begin"].view(np.uint64)[:4].tolist() == [0, 66, 132, 198] and (arrays["key_entry_begin"][8 * 4:] == 0xAB).all()
    assert arrays["key_trip_begin"].view(np.uint64)[:4].tolist() == [0, 11, 22, 33] and (arrays["key_trip_begin"][8 * 4:] == 0xAB).all()
    assert arrays["key_peak_lines"].view(np.uint32)[:3].tolist() == [6, 6, 6] and (arrays["key_peak_lines"][4 * 3:] == 0xAB).all() and (arrays["key_peak_line"][4 * 3:] == 0xAB).all()
    assert arrays["entry_window_lines"].view(np.uint32)[:198].tolist() == [1, 2, 3, 4, 5, 6] * 33
    for name, w in PER_ENTRY.items():
        assert (arrays[name][w * 198:] == 0xAB).all(), name
    assert arrays["entry_window_sum"].view(np.uint64)[:4 * 198].reshape(198, 4).tolist() == [[c, c, 0, 0] for c in (1, 2, 3, 4, 5, 6)] * 33
    assert (arrays["line_window_lines"][4 * 200:] == 0xAB).all() and arrays["line_window_lines"].view(np.uint32)[198:200].tolist() == [0, 0]
    assert sorted(arrays["entry_line"].view(np.uint32)[:198].tolist()) == list(range(198))
    fit = totals
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 198, 32)                          # one trip too few: nothing is written
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_trips" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 197, 33)                          # one entry too few
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_entries" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 197, 32, want=tuple(o for o in OUTS + KEY_OUTS if o not in PER_ENTRY and o not in PER_TRIP))
    assert rc == N.GX_OK and totals == fit                                                                     # ... bind the arrays of their family alone
    for name in PER_KEY:
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 198, 33, max_keys=2, want=(name,))
        assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_keys" in N.last_error(), name   # the per-key arrays are sized by max_keys
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 0, 0, want=())                    # the size query writes nothing
    assert rc == N.GX_OK and totals == fit and untouched(arrays)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 34, 198, 0, want=("trip_key", "key_trip_begin"))   # no trips: trip outputs are legal
    assert rc == N.GX_OK and totals["n_trips"] == 0 and (arrays["trip_key"] == 0xAB).all() and arrays["key_trip_begin"].view(np.uint64)[:4].tolist() == [0] * 4
    # the key table's own overflow: the window totals are zero
    rc, totals, arrays = raw_call(gorp, *batch(names(np.arange(65)), [1] * 65, values=[1] * 65), PV, 1, 1, 1024, 1024, max_keys=32)
    assert rc == N.GX_E_LIMIT and not totals["group"]["exact"] and totals["group"]["n_keys"] == 65 and untouched(arrays)
    assert [totals[name] for name in WINDOW_TOTALS] == [0, 0, 0, 0, 0, 0, NONE, NONE, 0, 0]
    # windows == NULL: the call is gx_group_lines bit for bit, the window totals zero
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 4, 198, 33, windows=False)
    assert rc == N.GX_OK and totals["group"]["n_keys"] == 3 and [totals[name] for name in WINDOW_TOTALS] == [0, 0, 0, 0, 0, 0, NONE, NONE, 0, 0]
    keys = gorp.group_lines(data, offsets, ids, caps, gorp.series_parts(PV)[0])
    assert totals["group"] == keys["totals"] and arrays["line_key"][:800].tobytes() == keys["line_key"].tobytes()
    assert arrays["key_lines"].view(np.uint64)[:3].tolist() == keys["lines"].tolist() and arrays["key_first_line"].view(np.uint32)[:3].tolist() == keys["first_line"].tolist()
    assert all((arrays[name] == 0xAB).all() for name in OUTS)


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


def test_device_pointers_poisoned_tails_the_size_query_and_a_second_call_on_another_stream(new_stream):
    import torch
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch(n=5000, seed=9)
    host = check(gorp, data, offsets, ids, caps, TWO_PARTS, 25, 4)
    t = host["totals"]
    m, nt, k, n = t["entries"], t["n_trips"], t["n_keys"], len(ids)
    assert nt > 20
    dev = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    d_data, d_off, d_ids, d_caps = dev(data), dev(offsets), dev(ids), dev(caps)
    streams = [new_stream(), new_stream()]
    torch.cuda.synchronize()
    args = (d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), TWO_PARTS, 25, 4)
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_windows_device(*args, max_keys=8, stream=streams[0].cuda_stream)                # the size query: every output NULL
    assert rc == N.GX_OK and totals == t
    runs = []
    mk = lambda count, dtype: torch.full((count + 4,), 0x5A, dtype=dtype, device="cuda")
    counts = {"entry_line": m, "entry_key": m, "entry_time": m, "entry_window_lines": m, "entry_window_sum": 4 * m, "key_entry_begin": k + 1, "key_peak_lines": k,
              "key_peak_line": k, "line_window_lines": n, "trip_key": nt, "trip_line": nt, "trip_time": nt, "trip_entry": nt, "key_trip_begin": k + 1}
    wide = ("entry_time", "entry_window_sum", "key_entry_begin", "trip_time", "key_trip_begin")
    for stream in streams:                                                                     # the second call right behind the first, on another stream
        out = {name: mk(c, torch.int64 if name in wide else torch.int32) for name, c in counts.items()}
        out.update(line_key=mk(n, torch.int32), key_lines=mk(k, torch.int64))
        with torch.cuda.stream(stream):
            rc, totals = gorp.group_windows_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                                   max_entries=m, max_trips=nt, stream=stream.cuda_stream, **{name + "_ptr": out[name].data_ptr() for name in OUTS})
        assert rc == N.GX_OK and totals == t
        runs.append(out)
    for stream in streams:
        stream.synchronize()                                                                   # the outputs are read after a stream wait
    x, y = [{name: a.cpu().numpy() for name, a in out.items()} for out in runs]
    assert all(x[name].tobytes() == y[name].tobytes() for name in x)
    for name, dtype in WINDOW_FIELDS:
        c = len(host[name])
        assert c == counts[name] and x[name][:c].view(dtype).tolist() == host[name].tolist() and (x[name][c:] == 0x5A).all(), name
    assert x["line_key"][:n].view(np.uint32).tolist() == host["line_key"].tolist() and x["key_lines"][:k].tolist() == host["lines"].tolist()
    sums = x["entry_window_sum"][:4 * m].reshape(m, 4)
    assert (x["entry_window_sum"][4 * m:] == 0x5A).all()
    for e, s in enumerate(host["entry_window_sum"]):
        assert int(sums[e, 0]) == s["numbers"] and (int(sums[e, 2]) << 64) + (int(sums[e, 1]) & (2 ** 64 - 1)) == s["sum"] and sums[e, 3] == 0
    # a capacity too small with device pointers: nothing is written, the key outputs included
    out = {"trip_key": mk(nt, torch.int32), "line_key": mk(n, torch.int32), "key_lines": mk(k, torch.int64)}
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_windows_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                               trip_key_ptr=out["trip_key"].data_ptr(), max_trips=nt - 1, stream=streams[0].cuda_stream)
    streams[0].synchronize()
    assert rc == N.GX_E_LIMIT and totals == t and all((a.cpu().numpy() == 0x5A).all() for a in out.values())


# ---------------------------------------------------------------------------
# 8. end to end: the syslog workload, extracted on the device, windows per host, and the same from raw text
# ---------------------------------------------------------------------------
def test_syslog_windows_per_host_end_to_end_and_from_raw_text():
    rules, meta = W.syslog_definition(4)
    gorp = Gorp.construct(rules)
    data, offsets, _ = W.syslog_lines(meta, 600, seed=11)
    data, offsets = np.asarray(data, np.uint8), np.asarray(offsets, np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids >= 0).sum() > 500
    for k in range(4):
        gorp.set_number_format(k, "ts", "iso8601", 3)
    parts = [("rule%d" % k, "host", "ts") for k in range(3)] + [("rule3", "host", "ts", "pid")]
    formats = {(k, gorp._extraction_and_group(k, "ts")[1]): ("iso8601", 3) for k in range(4)}
    both = gorp.series_parts(parts)
    runs = [check(gorp, data, offsets, ids, caps, parts, window, 3, formats=formats) for window in (0, 1_000, 10 ** 12)]
    peaks = [r["totals"]["peak_lines"] for r in runs]
    got = runs[1]
    # with a window longer than the log an entry's window is its key's entries so far
    assert peaks[0] <= peaks[1] <= peaks[2] == int(np.diff(runs[2]["key_entry_begin"].astype(np.int64)).max()) > 3 and got["totals"]["entries"] > 500
    assert runs[2]["totals"]["tripped_keys"] == runs[2]["totals"]["n_trips"] == int((np.diff(runs[2]["key_entry_begin"].astype(np.int64)) >= 3).sum())
    # the whole-file form: raw text in, the same keys and windows out, counts and n_lines as text_group_lines gives them
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))]
    raw = b"\n".join(lines) + b"\n"
    text, counts, n_lines = gorp.text_group_windows(raw, parts, 1_000, 3)
    keys, kcounts, kn = gorp.text_group_lines(raw, both[0])
    assert n_lines == kn == len(ids) and counts.tolist() == kcounts.tolist() and counts[:4].tolist() == [int((ids == k).sum()) for k in range(4)]
    assert text["totals"] == got["totals"] and text["entry_window_sum"] == got["entry_window_sum"] and text["keys"] == got["keys"] == keys["keys"]
    assert all(text[f].tobytes() == got[f].tobytes() for f in FIELDS + KEY_FIELDS) and text["totals"]["group"] == keys["totals"]


# ---------------------------------------------------------------------------
# 9. one large shape, and the flags on a mid-sized one
# ---------------------------------------------------------------------------
def test_half_a_million_lines_against_numpy():
    gorp = trivial_handle(1)
    n = 500_000
    key, t, matched = draw(n, seed=20)
    data, offsets, ids, caps = wide_batch(key, t, matched)
    window, threshold = 200_000_000, 12                                                        # 97 entries a key over 3 x 10^9: 6.5 a window
    want = np_windows(key, t, matched, window, threshold)
    got = gorp.group_windows(data, offsets, ids, caps, P, window, threshold, max_keys=8192, keys="csr")
    tt = got["totals"]
    assert tt["entries"] == tt["keyed"] == tt["lines"] == int(matched.sum()) and tt["n_keys"] == 5000
    assert (tt["first_time"], tt["last_time"]) == (int(t[matched].min()), int(t[matched].max()))
    for name, value in want["totals"].items():
        assert tt[name] == value, name
    for name, dtype in WINDOW_FIELDS:
        assert got[name].dtype == want[name].dtype == dtype and np.array_equal(got[name], want[name]), name
    assert 100 < tt["n_trips"] and tt["tripped_keys"] < tt["n_trips"] < tt["entries"] // 10 and tt["peak_lines"] > threshold


def test_all_digits_and_weak_hash_give_identical_results_on_a_mid_sized_case():
    gorp = trivial_handle(1)
    key, t, matched = draw(30_000, seed=21, n_keys=700, span=50_000_000)
    data, offsets, ids, caps = wide_batch(key, t, matched)
    base = gorp.group_windows(data, offsets, ids, caps, P, 3_000_000, 4, max_keys=1024, keys="csr")
    want = np_windows(key, t, matched, 3_000_000, 4)
    for name, dtype in WINDOW_FIELDS:
        assert np.array_equal(base[name], want[name]), name
    assert base["totals"]["n_trips"] == want["totals"]["n_trips"] > 100
    for hook in (dict(all_digits=True), dict(weak_hash=True), dict(weak_hash=True, all_digits=True)):
        again = gorp.group_windows(data, offsets, ids, caps, P, 3_000_000, 4, max_keys=1024, keys="csr", **hook)
        assert again["totals"] == base["totals"], hook
        for name in FIELDS + KEY_FIELDS:
            assert again[name].tobytes() == base[name].tobytes(), (hook, name)
