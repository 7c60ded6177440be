"""GPU tests of gx_group_sessions / gx_text_group_sessions: every key's lines ordered by a captured time and cut into sessions wherever
the time steps by more than max_gap -- the sessions ordered by (key number, begin), their entries, every key's run of sessions, the
session of every line.

Expected values come from tests/sessions_oracle.py -- a dict of lists sorted by (time, line) and a loop over Python's integers -- and
everything is compared bit for bit.  In every case the key outputs and totals["group"] are compared byte for byte with gx_group_lines'
on the same arguments, and the case runs once more under GX_BUCKET_ALL_DIGITS, under GX_GROUP_WEAK_HASH and under both, and must give the
same bytes.  Most batches are fabricated against handles of K identical, trivial extractions with three groups: a line is its key's
text, its time's text, its value's text and filler, its capture row made up here; the end-to-end case takes ids and rows from the
extraction itself.  The large shape is compared with a numpy restatement (lexsort + diff in uint64), which tests/test_sessions_host.py
compares with the oracle on smaller draws of the same generator.  The shapes are the smallest at which a pass can still go wrong: the
edges of a wave (64), of the sort's block and the scan's tile (2 048), and a session over three workgroups of 256 entries."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp
from number_oracle import KINDS
from sessions_oracle import INT64_MAX, INT64_MIN, NONE, SESSION_FIELDS, SESSION_TOTALS, batch, decode_parts, draw, group_sessions, np_sessions, same, wide_batch
from stats_oracle import SUM_SEQUENCES
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

BLOCK = 2048              # gx_scan.hpp's tile and the sort's block (BKT_BLOCK)
P = [(0, 0, 1)]           # extraction 0: group 0 the key, group 1 the time
PV = [(0, 0, 1, 2)]       # ... and group 2 measured
KEY_FIELDS = ("key_units", "key_offsets", "first_line", "lines", "line_key")
FIELDS = tuple(name for name, _ in SESSION_FIELDS)


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, max_gap, where=None, utf8=None, formats=None, hooks=True, **kw):
    """group_sessions against the restatement, every field; the keys against group_lines on the same arguments, byte for byte; then under
    the test hooks, the same bytes.  Returns what the call returned."""
    both = gorp.series_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    fm = {key: (KINDS[kind], scale) for key, (kind, scale) in (formats or {}).items()}
    want = group_sessions(data, offsets, ids, caps, decode_parts(both), gorp._sessions_gap(both, max_gap), decode_terms(terms), gorp.num_extractions, fm)
    got = gorp.group_sessions(data, offsets, ids, caps, both, max_gap, where=terms, utf8=utf8, **kw)
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
        again = gorp.group_sessions(data, offsets, ids, caps, both, max_gap, where=terms, utf8=utf8, **dict(kw, **hook))
        assert again["totals"] == got["totals"] and again["session_stats"] == got["session_stats"] and again["stats"] == got["stats"], hook
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
# 1. what a session is
# ---------------------------------------------------------------------------
def test_six_lines_two_keys_three_sessions():
    gorp = trivial_handle(1)
    got = check(gorp, *batch([b"u1", b"u2", b"u1", b"u1", b"u2", b"u1"], [100, 105, 130, 131, 104, 162], values=[1, 2, 3, 4, 5, 6]), PV, 30)
    assert got["keys"] == [b"u1", b"u2"] and got["session_key"].tolist() == [0, 0, 1]
    assert got["session_begin"].tolist() == [100, 162, 104] and got["session_end"].tolist() == [131, 162, 105]
    assert got["session_first_line"].tolist() == [0, 5, 4] and got["session_lines"].tolist() == [3, 1, 2]
    assert got["session_entry_begin"].tolist() == [0, 3, 4, 6] and got["key_session_begin"].tolist() == [0, 2, 3]
    assert got["entry_line"].tolist() == [0, 2, 3, 5, 4, 1] and got["line_session"].tolist() == [0, 2, 0, 0, 2, 1]
    assert [s["sum"] for s in got["session_stats"]] == [8, 6, 7] and [s["min"] for s in got["session_stats"]] == [1, 6, 2]
    t = got["totals"]
    assert (t["n_sessions"], t["entries"], t["longest_lines"], t["longest_duration"], t["first_time"], t["last_time"]) == (3, 6, 3, 31, 100, 162)


# ---------------------------------------------------------------------------
# 2. block edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_entries_at_the_edges_of_a_wave_a_sort_block_and_a_scan_tile(m):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(m)
    k = rng.integers(0, 5, m)
    t = rng.integers(-3000, 3000, m)
    keys, times = names(k), t.tolist()
    # a few lines that are no entries between them, so that the entries are not the lines
    for i in range(0, m, 97):
        keys.insert(i, b"k1")
        times.insert(i, [None, b"x"][i % 2])
    got = check(gorp, *batch(keys, times, values=list(range(len(keys)))), PV, 40)
    assert got["totals"]["entries"] == m and got["totals"]["n_sessions"] >= 1


def test_a_boundary_exactly_at_entry_2048_and_a_session_over_three_workgroups():
    gorp = trivial_handle(1)
    t = np.concatenate([np.arange(BLOCK), 10_000 + np.arange(700)])                  # one key: entries 0 .. 2047, a gap, 700 more
    rng = np.random.default_rng(1)
    order = rng.permutation(len(t))
    got = check(gorp, *batch(names(np.zeros(len(t), int)), t[order].tolist(), values=(order % 50 - 20).tolist()), PV, 1)
    assert got["session_entry_begin"].tolist() == [0, BLOCK, BLOCK + 700] and got["session_lines"].tolist() == [BLOCK, 700]
    assert [s["numbers"] for s in got["session_stats"]] == [BLOCK, 700]
    # key 1's one session of 700 entries lies at entries 100 .. 799: it begins in one workgroup of 256 entries and ends three further on
    k = np.concatenate([np.zeros(100, int), np.ones(700, int), np.full(100, 2)])
    t = np.concatenate([np.arange(100) * 5, np.arange(700), np.arange(100) * 5])
    order = rng.permutation(len(k))
    got = check(gorp, *batch(names(k[order]), t[order].tolist(), values=(order - 450).tolist()), PV, 1)
    s = got["session_lines"].tolist()
    assert s.count(700) == 1 and got["totals"]["n_sessions"] == 201 and got["totals"]["longest_lines"] == 700
    at = s.index(700)
    assert got["session_stats"][at]["numbers"] == 700 and got["session_stats"][at]["min"] is not None


def test_one_session_of_everything_every_entry_its_own_session_every_entry_its_own_key():
    gorp = trivial_handle(1)
    n = 2 * BLOCK + 77
    rng = np.random.default_rng(2)
    t = rng.permutation(n)
    got = check(gorp, *batch(names(np.zeros(n, int)), t.tolist(), values=(t - 2000).tolist()), PV, 1)        # distinct times one apart: one session
    assert got["totals"]["n_sessions"] == 1 and got["session_lines"].tolist() == [n] and got["totals"]["longest_duration"] == n - 1
    assert got["session_stats"][0]["sum"] == int((t - 2000).sum()) and (got["session_stats"][0]["min"], got["session_stats"][0]["max"]) == (-2000, n - 2001)
    got = check(gorp, *batch(names(np.zeros(n, int)), t.tolist(), values=(t - 2000).tolist()), PV, 0)        # max_gap = 0: every entry its own session
    assert got["totals"]["n_sessions"] == n and got["totals"]["longest_lines"] == 1 and got["totals"]["longest_duration"] == 0
    assert got["entry_line"].tolist() == np.argsort(t).tolist()
    got = check(gorp, *batch(names(np.arange(n)), [7] * n), P, INT64_MAX, max_keys=n, hooks=False)           # every entry its own key
    assert got["totals"]["n_sessions"] == n == got["totals"]["n_keys"] and got["key_session_begin"].tolist() == list(range(n + 1))
    got = check(gorp, *batch(names(np.arange(300)), [7] * 300), P, 5)                                          # ... and under the hooks
    assert got["session_key"].tolist() == list(range(300))


# ---------------------------------------------------------------------------
# 3. order
# ---------------------------------------------------------------------------
def test_descending_and_shuffled_times_ties_and_two_keys_interleaved():
    gorp = trivial_handle(1)
    got = check(gorp, *batch(names([0] * 300), list(range(3000, 0, -10))), P, 10)                              # descending: one session, reversed
    assert got["totals"]["n_sessions"] == 1 and got["entry_line"].tolist() == list(range(299, -1, -1))
    # ties in time inside a key: the order goes by input line, and no boundary opens even with max_gap = 0
    got = check(gorp, *batch(names([0, 1, 0, 0, 1, 0]), [50, 50, 50, 40, 50, 50]), P, 0)
    assert got["entry_line"].tolist() == [3, 0, 2, 5, 1, 4] and got["session_lines"].tolist() == [1, 3, 2]
    # two keys interleaved line by line: A every 10, B between them with one long pause -- A's gap must not see B's entries
    a = np.arange(200) * 10
    b = np.arange(200) * 10 + 5 + (np.arange(200) >= 100) * 100_000
    keys = [x for pair in zip(names([0] * 200), names([1] * 200)) for x in pair]
    times = [int(x) for pair in zip(a, b) for x in pair]
    got = check(gorp, *batch(keys, times), P, 10)
    assert got["session_lines"].tolist() == [200, 100, 100] and got["session_key"].tolist() == [0, 1, 1]
    rng = np.random.default_rng(3)
    k, t = rng.integers(0, 9, 3000), rng.integers(-40_000, 40_000, 3000)
    got = check(gorp, *batch(names(k), t.tolist(), values=rng.integers(-50, 50, 3000).tolist()), PV, 25)
    assert (np.diff(got["session_key"].astype(np.int64)) >= 0).all() and got["totals"]["n_sessions"] > 500


# ---------------------------------------------------------------------------
# 4. arithmetic
# ---------------------------------------------------------------------------
def test_the_corners_of_int64_negative_times_and_a_gap_of_exactly_max_gap():
    gorp = trivial_handle(1)
    got = check(gorp, *batch(names([0, 0]), [INT64_MAX, INT64_MIN]), P, INT64_MAX)
    assert got["totals"]["n_sessions"] == 2 and got["session_begin"].tolist() == [INT64_MIN, INT64_MAX] and got["totals"]["longest_duration"] == 0
    assert (got["totals"]["first_time"], got["totals"]["last_time"]) == (INT64_MIN, INT64_MAX)
    got = check(gorp, *batch(names([0, 0, 0]), [INT64_MAX, INT64_MIN, -1]), P, INT64_MAX)                  # -1 joins INT64_MIN (2^63 - 1 apart) ...
    assert got["session_lines"].tolist() == [2, 1] and got["totals"]["longest_duration"] == 2 ** 63 - 1
    got = check(gorp, *batch(names([0, 0, 0]), [INT64_MAX, INT64_MIN, 0]), P, INT64_MAX)                   # ... and 0 joins INT64_MAX
    assert got["session_lines"].tolist() == [1, 2] and got["session_begin"].tolist() == [INT64_MIN, 0]
    got = check(gorp, *batch(names([0] * 6), [-100, -70, -39, -9, 21, 52]), P, 30)                          # 30, 31, 30, 30, 31
    assert got["session_begin"].tolist() == [-100, -39, 52] and got["session_end"].tolist() == [-70, 21, 52]
    got = check(gorp, *batch(names([0] * 6), [-100, -70, -39, -9, 21, 52]), P, 31)
    assert got["totals"]["n_sessions"] == 1
    got = check(gorp, *batch(names([0] * 3), [5, 6, 8]), P, 0)
    assert got["totals"]["n_sessions"] == 3
    # the values' own corners: a session whose only number is INT64_MAX, one whose only number is INT64_MIN, one with both and one with none
    got = check(gorp, *batch(names([0] * 6), [0, 100, 200, 201, 300, 301], values=[INT64_MAX, INT64_MIN, INT64_MIN, INT64_MAX, None, b"x"]), PV, 10)
    assert [(s["min"], s["max"], s["sum"]) for s in got["session_stats"]] == [(INT64_MAX, INT64_MAX, INT64_MAX), (INT64_MIN, INT64_MIN, INT64_MIN), (INT64_MIN, INT64_MAX, -1),
                                                                              (None, None, 0)]


@pytest.mark.parametrize("name", sorted(SUM_SEQUENCES))
def test_128_bit_sums_per_session(name):
    gorp = trivial_handle(1)
    values = [v for count, v in SUM_SEQUENCES[name] for _ in range(count)]
    assert len(values) == 70000
    rng = np.random.default_rng(3)
    rng.shuffle(values)
    which = rng.integers(0, 3, len(values))
    times = (rng.integers(0, 2, len(values)) * 1000 + rng.integers(0, 50, len(values))).tolist()         # two sessions per key
    got = check(gorp, *batch(names(which), times, values=values), PV, 100, hooks=False)
    assert got["totals"]["n_sessions"] == 6 and sum(s["sum"] for s in got["session_stats"]) == sum(values)
    assert any(not INT64_MIN <= s["sum"] <= INT64_MAX for s in got["session_stats"])


# ---------------------------------------------------------------------------
# 5. classes, parts, terms
# ---------------------------------------------------------------------------
def test_each_class_of_keyed_line_adds_up_and_a_part_without_a_number():
    gorp = trivial_handle(2)
    keys = [b"x", b"x", b"y", b"x", None, b"y", b"y", b"z", b"x", b"y"]
    times = [5, -2 ** 63, None, b"12x", 7, b"", 6, 8, 5, 5]
    ids = [0, 0, 0, 0, 0, 0, 1, 1, -1, 0]
    data, offsets, ids, caps = batch(keys, times, values=[1, 2, 3, 4, 5, 6, 7, None, 9, b"q"], lengths=[9] * 10, ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, 1, 2)], 1)
    t = got["totals"]
    assert (t["lines"], t["keyed"], t["unset"], t["entries"], t["number_unset"], t["not_numbers"]) == (9, 8, 1, 5, 1, 2)
    assert got["keys"] == [b"x", b"y", b"z"] and got["session_key"].tolist() == [0, 0, 1, 2] and got["line_session"].tolist() == [1, 0, NONE, NONE, NONE, NONE, 2, 3, NONE, 2]
    # number_groups = -1 for one of two parts: extraction 1's lines have a key and no time; two extractions share the keys
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 2), (1, 0, None, 2)], 1)
    t = got["totals"]
    assert (t["keyed"], t["entries"], t["number_unset"]) == (8, 3, 3) and got["key_session_begin"].tolist() == [0, 2, 3, 3]
    # no part at all, and no line at all: all zeros, the bounds' one entry, no line has a session
    got = check(gorp, data, offsets, ids, caps, [], 1)
    assert got["totals"]["n_sessions"] == 0 and got["key_session_begin"].tolist() == [0] and got["session_entry_begin"].tolist() == [0]
    assert set(got["line_session"].tolist()) == {NONE}
    got = check(gorp, *batch([], []), P, 1)
    assert got["totals"]["n_sessions"] == 0 and len(got["line_session"]) == 0 and got["key_session_begin"].tolist() == [0] and got["session_entry_begin"].tolist() == [0]
    got = check(gorp, *batch([b"a", b"b"], [None, b"x"]), P, 1)                               # keyed lines, none of them an entry
    assert got["totals"]["n_sessions"] == 0 and got["key_session_begin"].tolist() == [0, 0, 0] and got["line_session"].tolist() == [NONE, NONE]
    assert [got["totals"][name] for name in SESSION_TOTALS] == [0, 0, 1, 1, 0, 0, 0, 0]


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
    got = check(gorp, data, offsets, pack(ids, caps, rows), None, TWO_PARTS, 30)
    assert got["totals"]["n_sessions"] > 20 and got["totals"]["number_unset"] > 0 and got["totals"]["not_numbers"] > 0 and got["totals"]["unset"] > 0


def test_offsets64_utf16_utf8_bytes_and_where_terms():
    gorp = trivial_handle(2)
    base = check(gorp, *mixed_batch(), TWO_PARTS, 30)
    for kw, utf8 in ((dict(offsets_dtype=np.uint64), None), (dict(dtype=np.uint16), None), (dict(dtype=np.uint16, offsets_dtype=np.uint64), None), ({}, "bytes")):
        got = check(gorp, *mixed_batch(**kw), TWO_PARTS, 30, utf8=utf8)
        assert {k: got["totals"][k] for k in SESSION_TOTALS} == {k: base["totals"][k] for k in SESSION_TOTALS} and got["session_stats"] == base["session_stats"]
        assert all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)
    got = check(gorp, *mixed_batch(), TWO_PARTS, 30, where=[(0, 2, ">=", 500), (1, 2, "<", 0)])
    assert 0 < got["totals"]["lines"] < 300 and got["totals"]["n_sessions"] > 10


def test_number_formats_iso8601_with_max_gap_in_milliseconds():
    gorp = trivial_handle(1, tag="iso")
    gorp.set_number_format(0, 1, "iso8601", 3)
    gorp.set_number_format(0, 2, "decimal", 2)
    stamps = [b"2026-01-03T00:00:01.123Z", b"2026-01-03T00:00:31.123Z", b"2026-01-03T00:01:01.124Z", b"2026-01-02T23:59:59.999Z", b"2026-01-03T01:00:00+01:00",
              b"yesterday", None, b"2026-01-03T00:01:30Z"]
    keys = [b"GET", b"PUT", b"GET", b"GET", b"PUT", b"GET", b"PUT", b"GET"]
    values = [b"0.25", b"1", b"-1.00", b"2.50", b"x", b"1", b"1", b"0.5"]
    formats = {(0, 1): ("iso8601", 3), (0, 2): ("decimal", 2)}
    got = check(gorp, *batch(keys, stamps, values=values), PV, 30_000, formats=formats)
    assert got["session_key"].tolist() == [0, 0, 1, 1] and got["session_lines"].tolist() == [2, 2, 1, 1] and got["entry_line"].tolist() == [3, 0, 2, 7, 4, 1]
    assert [s["sum"] for s in got["session_stats"]] == [275, -50, 0, 100] and got["totals"]["not_numbers"] == 1 and got["totals"]["number_unset"] == 1
    assert got["totals"]["longest_duration"] == 28_876 and got["session_stats"][2]["not_numbers"] == 1
    got = check(gorp, *batch(keys, stamps, values=values), PV, 60_001, formats=formats)
    assert got["session_lines"].tolist() == [4, 2]


# ---------------------------------------------------------------------------
# 7. the calling forms
# ---------------------------------------------------------------------------
OUTS = ("session_key", "session_begin", "session_end", "session_first_line", "session_lines", "session_stats", "session_entry_begin", "key_session_begin",
        "entry_line", "line_session")
KEY_OUTS = ("key_units", "key_offsets", "key_first_line", "key_lines", "key_stats", "line_key")


def raw_call(gorp, data, offsets, ids, caps, parts, max_gap, max_sessions, max_entries=None, max_keys=64, want=OUTS + KEY_OUTS, poison=0xAB, sessions=True):
    """gx_group_sessions itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p, numbers = gorp.series_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n = len(offsets) - 1
    max_entries = n if max_entries is None else max_entries
    ms, me = max_sessions, max_entries
    sizes = {"session_key": 4 * (ms + 8), "session_begin": 8 * (ms + 8), "session_end": 8 * (ms + 8), "session_first_line": 4 * (ms + 8), "session_lines": 8 * (ms + 8),
             "session_stats": 64 * (ms + 8), "session_entry_begin": 8 * (ms + 9), "key_session_begin": 8 * (max_keys + 9), "entry_line": 4 * (me + 8),
             "line_session": 4 * (n + 8), "key_units": 4096, "key_offsets": 4 * (max_keys + 9), "key_first_line": 4 * (max_keys + 8), "key_lines": 8 * (max_keys + 8),
             "key_stats": 64 * (max_keys + 8), "line_key": 4 * (n + 8)}
    arrays = {name: np.full(size, poison, np.uint8) for name, size in sizes.items()}
    ptr = lambda name: arrays[name].ctypes.data if name in want and (p.has_values or not name.endswith("_stats")) else None
    keys = N.gx_group_out(ptr("key_units"), 4096, ptr("key_offsets"), ptr("key_first_line"), ptr("key_lines"), ptr("key_stats"), ptr("line_key"), max_keys)
    out = N.gx_sessions_out(*[ptr(name) for name in OUTS], max_sessions, max_entries)
    totals = N.gx_sessions_totals()
    rc = N.lib().gx_group_sessions(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, numbers, max_gap, None, 0, 0,
                                   C.byref(keys), C.byref(out) if sessions else None, C.byref(totals), C.byref(o))
    return rc, Gorp._sessions_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a == poison).all() for a in arrays.values())


def test_capacities_poisoned_outputs_the_size_query_and_sessions_null():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(33)
    cell = rng.permutation(np.repeat(np.arange(33), 6))                                       # 33 sessions of 6 entries: 3 keys x 11 sessions
    data, offsets, ids, caps = batch(names(cell % 3) + [b"k0", b"k1"], (cell // 3 * 100).tolist() + [None, b"x"], values=[1] * 200)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 33, max_entries=198)                 # exactly sufficient
    assert rc == N.GX_OK and (totals["n_sessions"], totals["entries"], totals["number_unset"], totals["not_numbers"], totals["longest_lines"]) == (33, 198, 1, 1, 6)
    assert arrays["session_key"].view(np.uint32)[:33].tolist() == sorted((cell % 3).tolist())[::6] and (arrays["session_key"][4 * 33:] == 0xAB).all()
    assert arrays["session_begin"].view(np.int64)[:11].tolist() == list(range(0, 1100, 100)) and (arrays["session_begin"][8 * 33:] == 0xAB).all()
    assert arrays["session_entry_begin"].view(np.uint64)[:34].tolist() == list(range(0, 199, 6)) and (arrays["session_entry_begin"][8 * 34:] == 0xAB).all()
    assert arrays["key_session_begin"].view(np.uint64)[:4].tolist() == [0, 11, 22, 33] and (arrays["key_session_begin"][8 * 4:] == 0xAB).all()
    assert (arrays["entry_line"][4 * 198:] == 0xAB).all() and (arrays["line_session"][4 * 200:] == 0xAB).all() and (arrays["session_stats"][64 * 33:] == 0xAB).all()
    assert sorted(arrays["entry_line"].view(np.uint32)[:198].tolist()) == list(range(198))
    fit = totals
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 32, max_entries=198)                 # one session too few: nothing is written
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_sessions" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 33, max_entries=197)                 # one entry too few
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_entries" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 33, max_entries=197, want=tuple(o for o in OUTS + KEY_OUTS if o != "entry_line"))
    assert rc == N.GX_OK and totals == fit                                                                     # ... binds entry_line alone
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 33, max_keys=2, want=("key_session_begin",))
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_keys" in N.last_error()         # key_session_begin is sized by max_keys
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 0, max_entries=0, want=())           # the size query writes nothing
    assert rc == N.GX_OK and totals == fit and untouched(arrays)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 0, want=("line_session", "key_session_begin", "entry_line"))   # no per-session array
    assert rc == N.GX_OK and sorted(set(arrays["line_session"].view(np.uint32)[:200].tolist())) == list(range(33)) + [NONE]
    # the key table's own overflow: the session totals are zero
    rc, totals, arrays = raw_call(gorp, *batch(names(np.arange(65)), [1] * 65, values=[1] * 65), PV, 1, 1024, max_keys=32)
    assert rc == N.GX_E_LIMIT and not totals["group"]["exact"] and totals["group"]["n_keys"] == 65 and untouched(arrays)
    assert [totals[name] for name in SESSION_TOTALS] == [0] * 8
    # sessions == NULL: the call is gx_group_lines bit for bit, the session totals zero
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, PV, 50, 33, sessions=False)
    assert rc == N.GX_OK and totals["group"]["n_keys"] == 3 and [totals[name] for name in SESSION_TOTALS] == [0] * 8
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
    host = check(gorp, data, offsets, ids, caps, TWO_PARTS, 3)
    t = host["totals"]
    s, m, k, n = t["n_sessions"], t["entries"], t["n_keys"], len(ids)
    dev = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    d_data, d_off, d_ids, d_caps = dev(data), dev(offsets), dev(ids), dev(caps)
    streams = [new_stream(), new_stream()]
    torch.cuda.synchronize()
    args = (d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), TWO_PARTS, 3)
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_sessions_device(*args, max_keys=8, stream=streams[0].cuda_stream)               # the size query: every output NULL
    assert rc == N.GX_OK and totals == t
    runs = []
    mk = lambda count, dtype: torch.full((count + 4,), 0x5A, dtype=dtype, device="cuda")
    for stream in streams:                                                                     # the second call right behind the first, on another stream
        out = {"session_key": mk(s, torch.int32), "session_begin": mk(s, torch.int64), "session_end": mk(s, torch.int64), "session_first_line": mk(s, torch.int32),
               "session_lines": mk(s, torch.int64), "session_stats": mk(8 * s, torch.int64), "session_entry_begin": mk(s + 1, torch.int64),
               "key_session_begin": mk(k + 1, torch.int64), "entry_line": mk(m, torch.int32), "line_session": mk(n, torch.int32), "line_key": mk(n, torch.int32),
               "key_lines": mk(k, torch.int64)}
        with torch.cuda.stream(stream):
            rc, totals = gorp.group_sessions_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                                    max_sessions=s, max_entries=m, stream=stream.cuda_stream, **{name + "_ptr": out[name].data_ptr() for name in OUTS})
        assert rc == N.GX_OK and totals == t
        runs.append(out)
    for stream in streams:
        stream.synchronize()                                                                   # the outputs are read after a stream wait
    x, y = [{name: a.cpu().numpy() for name, a in out.items()} for out in runs]
    assert all(x[name].tobytes() == y[name].tobytes() for name in x)
    for name, dtype in SESSION_FIELDS:
        c = len(host[name])
        assert x[name][:c].view(dtype).tolist() == host[name].tolist() and (x[name][c:] == 0x5A).all(), name
    assert x["line_key"][:n].view(np.uint32).tolist() == host["line_key"].tolist() and x["key_lines"][:k].tolist() == host["lines"].tolist()
    stats = x["session_stats"][:8 * s].reshape(s, 8)
    assert (x["session_stats"][8 * s:] == 0x5A).all()
    for j, st in enumerate(host["session_stats"]):
        assert stats[j, :4].tolist() == [st["lines"], st["numbers"], st["unset"], st["not_numbers"]]
        assert st["numbers"] == 0 or (int(stats[j, 4]), int(stats[j, 5])) == (st["min"], st["max"])
        assert (int(stats[j, 7]) << 64) + (int(stats[j, 6]) & (2 ** 64 - 1)) == st["sum"]
    # a capacity too small with device pointers: nothing is written, the key outputs included
    out = {"session_key": mk(s, torch.int32), "line_key": mk(n, torch.int32), "key_lines": mk(k, torch.int64)}
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_sessions_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                                session_key_ptr=out["session_key"].data_ptr(), max_sessions=s - 1, stream=streams[0].cuda_stream)
    streams[0].synchronize()
    assert rc == N.GX_E_LIMIT and totals == t and all((a.cpu().numpy() == 0x5A).all() for a in out.values())


# ---------------------------------------------------------------------------
# 8. end to end: the syslog workload, extracted on the device, sessions per host, and the same from raw text
# ---------------------------------------------------------------------------
def test_syslog_sessions_per_host_end_to_end_and_from_raw_text():
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
    runs = [check(gorp, data, offsets, ids, caps, parts, gap, formats=formats) for gap in (0, 1_000, 10 ** 12)]
    sizes = [r["totals"]["n_sessions"] for r in runs]
    got = runs[1]
    t = got["totals"]
    # with a gap longer than the log a key that has an entry has one session
    assert sizes[0] >= sizes[1] >= sizes[2] == int(np.count_nonzero(np.diff(runs[2]["key_session_begin"].astype(np.int64)))) > 1
    assert sizes[2] <= t["n_keys"] and t["entries"] > 500 and sizes[0] > sizes[2]
    # the whole-file form: raw text in, the same keys and sessions out, counts and n_lines as text_group_lines gives them
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))]
    raw = b"\n".join(lines) + b"\n"
    text, counts, n_lines = gorp.text_group_sessions(raw, parts, 1_000)
    keys, kcounts, kn = gorp.text_group_lines(raw, both[0])
    assert n_lines == kn == len(ids) and counts.tolist() == kcounts.tolist() and counts[:4].tolist() == [int((ids == k).sum()) for k in range(4)]
    assert text["totals"] == got["totals"] and text["session_stats"] == got["session_stats"] and text["keys"] == got["keys"] == keys["keys"]
    assert all(text[f].tobytes() == got[f].tobytes() for f in FIELDS + KEY_FIELDS) and text["totals"]["group"] == keys["totals"]


# ---------------------------------------------------------------------------
# 9. one large shape
# ---------------------------------------------------------------------------
def test_half_a_million_lines_against_numpy():
    gorp = trivial_handle(1)
    n = 500_000
    key, t, matched = draw(n, seed=20)
    data, offsets, ids, caps = wide_batch(key, t, matched)
    max_gap = 100_000_000                                                                      # 97 entries a key over 3 x 10^9: a few sessions per key
    want = np_sessions(key, t, matched, max_gap)
    got = gorp.group_sessions(data, offsets, ids, caps, P, max_gap, max_keys=8192, keys="csr")
    tt = got["totals"]
    assert tt["n_sessions"] == len(want["session_key"]) and tt["entries"] == tt["keyed"] == tt["lines"] == int(matched.sum()) and tt["n_keys"] == 5000
    assert (tt["first_time"], tt["last_time"]) == (int(t[matched].min()), int(t[matched].max())) and tt["longest_lines"] == int(want["session_lines"].max())
    assert tt["longest_duration"] == int((want["session_end"] - want["session_begin"]).max())
    for name, dtype in SESSION_FIELDS:
        assert got[name].dtype == want[name].dtype == dtype and np.array_equal(got[name], want[name]), name
    assert 3 * 5000 < tt["n_sessions"] < 8 * 5000 and tt["longest_lines"] > 64
