"""GPU tests of gx_group_spans / gx_text_group_spans: every key's BEGIN and END lines paired in input order -- the spans ordered by (key
number, end line), their sides, exact durations and classes, every key's run of spans, its stats and the begin it leaves open, the span
and the state of every line.

Expected values come from tests/spans_oracle.py -- ONE pass in input order with a dict of the open begins, put and remove, durations in
Python's integers -- and everything is compared bit for bit.  In every case the key outputs and totals["group"] are compared byte for
byte with gx_group_lines' on the same arguments, the case runs once more under GX_BY_KEY_ALL_DIGITS, under GX_GROUP_WEAK_HASH and under
both and must give the same bytes, and the identities of include/gorp_hip.h are asserted.  Most batches are fabricated against handles
of K identical, trivial extractions with three groups: a line is its key's text, its time's text, its value's text and filler, its
capture row made up here, and its ROLE is its extraction's (extraction 0 begins, extraction 1 ends); the end-to-end case takes ids and
rows from the extraction itself.  The large shape is compared with a numpy restatement (stable argsort + shifted compares), which
tests/test_spans_host.py compares with the oracle on smaller draws of the same generator.  The shapes are the smallest at which a pass
can still go wrong: an entry reads the entries before and behind it, across the edges of a wave (64), of a workgroup (256) and of the
sort's block and the scan's tile (2 048)."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp
from number_oracle import KINDS
from spans_oracle import (INT64_MAX, INT64_MIN, NONE, SPAN_FIELDS, SPAN_TOTALS, batch, decode_parts, draw, group_spans, identities, np_spans, same,
                          wide_batch)
from stats_oracle import SUM_SEQUENCES
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

BLOCK = 2048              # gx_scan.hpp's tile and the sort's block (BKT_BLOCK)
SP = [(0, 0, 1, "begin"), (1, 0, 1, "end")]            # extraction 0 begins, extraction 1 ends: group 0 the key, group 1 the time
SPV = [(0, 0, 1, "begin", 2), (1, 0, 1, "end", 2)]     # ... and group 2 measured (the keys' stats; the terms read it)
KEY_FIELDS = ("key_units", "key_offsets", "first_line", "lines", "line_key")
FIELDS = tuple(name for name, _ in SPAN_FIELDS)


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, where=None, utf8=None, formats=None, hooks=True, **kw):
    """group_spans against the oracle, every field; the keys against group_lines on the same arguments, byte for byte; then under the
    test hooks, the same bytes.  Returns what the call returned."""
    three = gorp.span_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    fm = {key: (KINDS[kind], scale) for key, (kind, scale) in (formats or {}).items()}
    want = group_spans(data, offsets, ids, caps, decode_parts(three), decode_terms(terms), gorp.num_extractions, fm)
    got = gorp.group_spans(data, offsets, ids, caps, three, where=terms, utf8=utf8, **kw)
    same(got, want)
    t = got["totals"]
    keys = gorp.group_lines(data, offsets, ids, caps, three[0], where=terms, utf8=utf8, max_keys=kw.get("max_keys"))
    assert t["group"] == keys["totals"] and got["stats"] == keys["stats"] and got["keys"] == keys["keys"]
    for name in KEY_FIELDS:
        assert got[name].dtype == keys[name].dtype and got[name].tobytes() == keys[name].tobytes(), name
    for hook in ([dict(all_digits=True), dict(weak_hash=True), dict(weak_hash=True, all_digits=True)] if hooks else []):
        if hook.get("weak_hash") and t["n_keys"] > 4096:
            continue
        again = gorp.group_spans(data, offsets, ids, caps, three, where=terms, utf8=utf8, **dict(kw, **hook))
        assert again["totals"] == got["totals"] and again["key_span_stats"] == got["key_span_stats"] and again["stats"] == got["stats"], hook
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
    return [None if k is None else b"k%d" % int(k) for k in numbers]


def roles_batch(keys, roles, times=None, **kw):
    """batch() of lines whose extraction is their role: roles a string of B, E and - (the line matches nothing)"""
    ids = [{"B": 0, "E": 1, "-": -1}[r] for r in roles]
    return batch(keys, list(range(len(keys))) if times is None else times, ids=ids, **kw)


# ---------------------------------------------------------------------------
# 1. what a span is
# ---------------------------------------------------------------------------
def test_b_b_e_e_on_one_key_one_span_one_superseded_one_orphan():
    gorp = trivial_handle(2)
    got = check(gorp, *roles_batch([b"r1"] * 4, "BBEE", [100, 110, 140, 150]), SP)
    assert got["line_state"].tolist() == [3, 1, 2, 5] and got["line_span"].tolist() == [NONE, 0, 0, NONE]
    assert (got["span_key"].tolist(), got["span_begin_line"].tolist(), got["span_end_line"].tolist()) == ([0], [1], [2])
    assert (got["span_begin"].tolist(), got["span_end"].tolist(), got["span_duration"].tolist(), got["span_class"].tolist()) == ([110], [140], [30], [0])
    assert got["key_span_begin"].tolist() == [0, 1] and got["key_open_line"].tolist() == [NONE]
    t = got["totals"]
    assert [t[name] for name in SPAN_TOTALS] == [1, 2, 2, 1, 0, 1, 0] and t["durations"] == {"lines": 1, "numbers": 1, "unset": 0, "not_numbers": 0, "min": 30, "max": 30, "sum": 30}


def test_every_state_in_nine_lines_two_keys_interleaved_and_neighbours_of_two_keys():
    gorp = trivial_handle(2)
    #       line:   0      1      2      3      4      5      6      7      8
    keys = [b"a", b"b", b"a", None, b"b", b"a", b"a", b"b", b"a"]
    got = check(gorp, *roles_batch(keys, "BBB-EEEEB", [10, 20, 30, 0, 15, 70, 80, 95, 99]), SP)
    assert got["keys"] == [b"a", b"b"]
    assert got["line_state"].tolist() == [3, 1, 1, 0, 2, 2, 5, 5, 4]                      # every state: a is B B E E B, b is B E E
    assert got["span_key"].tolist() == [0, 1] and got["span_begin_line"].tolist() == [2, 1] and got["span_end_line"].tolist() == [5, 4]
    assert got["span_duration"].tolist() == [40, -5] and got["line_span"].tolist() == [NONE, 1, 0, NONE, 1, 0, NONE, NONE, NONE]
    assert got["key_span_begin"].tolist() == [0, 1, 2] and got["key_open_line"].tolist() == [8, NONE]
    assert [s["sum"] for s in got["key_span_stats"]] == [40, -5]
    # two keys interleaved line by line do not see each other: x is B E B E ..., y is E B E B ...
    n = 200
    keys = [k for pair in zip([b"x"] * n, [b"y"] * n) for k in pair]
    roles = "".join("BE"[i % 2] + "EB"[i % 2] for i in range(n))
    got = check(gorp, *roles_batch(keys, roles), SP)
    assert got["totals"]["n_spans"] == n // 2 + (n // 2 - 1) and got["totals"]["orphan_ends"] == 1 and got["totals"]["left_open"] == 1
    assert got["span_key"].tolist() == [0] * (n // 2) + [1] * (n // 2 - 1) and set(got["span_duration"].tolist()) == {2}
    # a key whose last entry is a BEGIN sits next, in key order, to a key whose first entry is an END: they must NOT pair
    got = check(gorp, *roles_batch([b"p", b"q", b"p", b"q"], "EEBE"), SP)
    assert got["totals"]["n_spans"] == 0 and got["line_state"].tolist() == [5, 5, 4, 5] and got["key_open_line"].tolist() == [2, NONE]
    got = check(gorp, *roles_batch([b"p", b"q"], "BE"), SP)
    assert got["totals"]["n_spans"] == 0 and got["line_state"].tolist() == [4, 5] and got["key_span_begin"].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# 2. edges: an entry reads its two neighbours across waves, workgroups, sort blocks and scan tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_entries_at_the_edges_of_a_wave_a_workgroup_a_sort_block_and_a_scan_tile(m):
    gorp = trivial_handle(2)
    rng = np.random.default_rng(m)
    keys = names(rng.integers(0, 5, m))
    roles = list(rng.choice(list("BE"), m))
    times = rng.integers(-3000, 3000, m).tolist()
    # a few lines that are no entries between them -- no match, or a key that is unset -- so that the entries are not the lines
    for i in range(0, m, 97):
        keys.insert(i, [b"k1", None][i % 2])
        roles.insert(i, "-B"[i % 2])
        times.insert(i, 5)
    got = check(gorp, *roles_batch(keys, "".join(roles), times), SP)
    assert got["totals"]["keyed"] == m and got["totals"]["begins"] + got["totals"]["ends"] == m


def test_a_pair_exactly_across_entries_63_64_255_256_and_2047_2048():
    gorp = trivial_handle(2)
    m = BLOCK + 100
    # one key, so that entry e is line e: every entry an END but a BEGIN at the last entry of a wave, of a workgroup and of a sort block /
    # scan tile, whose END is the first entry of the next
    roles = ["E"] * m
    for e in (63, 255, BLOCK - 1):
        roles[e] = "B"
    got = check(gorp, *roles_batch(names([0] * m), "".join(roles)), SP)
    assert got["span_begin_line"].tolist() == [63, 255, BLOCK - 1] and got["span_end_line"].tolist() == [64, 256, BLOCK]
    assert got["totals"]["n_spans"] == 3 and got["totals"]["orphan_ends"] == m - 6 and got["span_duration"].tolist() == [1, 1, 1]
    # the same with a KEY boundary at those places: key j's last entry is a BEGIN, key j + 1's first an END -- no span.  The keys' entries
    # number 64, 192, 1792 and 100, so the runs end at entries 64, 256 and 2048 of the (key, line) order; the lines are interleaved
    sizes = [64, 192, BLOCK - 256, 100]
    rng = np.random.default_rng(7)
    rest = np.concatenate([np.full(size - 1, j) for j, size in enumerate(sizes)])
    rng.shuffle(rest)
    k = np.concatenate([np.arange(4), rest])                                                 # (key numbers by first appearance: 0, 1, 2, 3)
    last = {j: int(np.flatnonzero(k == j)[-1]) for j in range(4)}
    roles = "".join("B" if last[int(k[i])] == i else "E" for i in range(len(k)))
    got = check(gorp, *roles_batch(names(k), roles), SP)
    t = got["totals"]
    assert (t["n_spans"], t["left_open"], t["begins"], t["orphan_ends"]) == (0, 4, 4, len(k) - 4) and got["key_open_line"].tolist() == [last[j] for j in range(4)]
    assert got["lines"].tolist() == sizes and got["key_span_begin"].tolist() == [0] * 5


def test_one_key_of_everything_every_entry_its_own_key_all_begins_all_ends():
    gorp = trivial_handle(2)
    n = 2 * BLOCK + 77
    got = check(gorp, *roles_batch(names([0] * n), "BE" * (n // 2) + "B", (np.arange(n) * 3).tolist()), SP)       # B E B E ... B
    t = got["totals"]
    assert (t["n_spans"], t["left_open"], t["superseded"], t["orphan_ends"]) == (n // 2, 1, 0, 0) and got["key_open_line"].tolist() == [n - 1]
    assert got["span_end_line"].tolist() == list(range(1, n, 2)) and t["durations"]["sum"] == 3 * (n // 2) and got["key_span_stats"][0] == t["durations"]
    got = check(gorp, *roles_batch(names(np.arange(n)), "BE" * (n // 2) + "B"), SP, max_keys=n, hooks=False)       # every entry its own key
    t = got["totals"]
    assert (t["n_spans"], t["left_open"], t["orphan_ends"], t["n_keys"]) == (0, n // 2 + 1, n // 2, n)
    assert got["key_open_line"].tolist() == [i if i % 2 == 0 else NONE for i in range(n)] and got["key_span_begin"].tolist() == [0] * (n + 1)
    got = check(gorp, *roles_batch(names(np.arange(300)), "EB" * 150), SP)                                         # ... and under the hooks
    assert got["totals"]["left_open"] == 150 and got["totals"]["orphan_ends"] == 150
    rng = np.random.default_rng(4)
    k = rng.integers(0, 7, 700)
    got = check(gorp, *roles_batch(names(k), "B" * 700), SP)                                                       # all BEGINs
    t = got["totals"]
    assert (t["n_spans"], t["begins"], t["ends"], t["left_open"], t["superseded"]) == (0, 700, 0, 7, 693)
    got = check(gorp, *roles_batch(names(k), "E" * 700), SP)                                                       # all ENDs
    t = got["totals"]
    assert (t["n_spans"], t["begins"], t["ends"], t["orphan_ends"]) == (0, 0, 700, 700) and set(got["key_open_line"].tolist()) == {NONE}


# ---------------------------------------------------------------------------
# 3. arithmetic
# ---------------------------------------------------------------------------
def test_the_corners_of_int64_from_text_and_negative_durations():
    gorp = trivial_handle(2)
    # (begin, end) per key.  INT64_MAX - (-1) is 2^63, one more than int64 holds: out of range like the two full swings; the largest
    # duration that fits from either end is 2^63 - 1, the smallest -2^63
    pairs = [(INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (-1, INT64_MAX), (0, INT64_MAX), (0, INT64_MIN), (INT64_MIN, -1), (5, 5), (INT64_MAX, INT64_MAX),
             (1, INT64_MIN), (INT64_MIN, 0)]
    keys = [k for j in range(len(pairs)) for k in (b"k%d" % j, b"k%d" % j)]
    got = check(gorp, *roles_batch(keys, "BE" * len(pairs), [t for pair in pairs for t in pair]), SP)
    assert got["span_class"].tolist() == [2, 2, 2, 0, 0, 0, 0, 0, 2, 2]
    assert got["span_duration"].tolist() == [0, 0, 0, INT64_MAX, INT64_MIN, INT64_MAX, 0, 0, 0, 0]
    assert got["span_begin"].tolist() == [b for b, _ in pairs] and got["span_end"].tolist() == [e for _, e in pairs]     # the sides stay the numbers they are
    t = got["totals"]
    assert t["out_of_range"] == 5 and t["durations"] == {"lines": 10, "numbers": 5, "unset": 0, "not_numbers": 5, "min": INT64_MIN, "max": INT64_MAX,
                                                          "sum": 2 * INT64_MAX + INT64_MIN}
    # negative durations -- the end stamped earlier than the begin -- are numbers like any other
    got = check(gorp, *roles_batch(names([0] * 6), "BEBEBE", [100, 40, -5, -6, 0, -2 ** 40]), SP)
    assert got["span_duration"].tolist() == [-60, -1, -2 ** 40] and got["totals"]["durations"]["min"] == -2 ** 40 and got["totals"]["durations"]["max"] == -1


def test_sides_unset_unparsable_both_and_a_part_without_a_number_group():
    gorp = trivial_handle(2)
    times = [None, 7, 3, None, b"x", 9, 2, b"1e3", None, b"-", b"", 4, 10, 30]
    got = check(gorp, *roles_batch(names([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]), "BE" * 7, times), SP)
    assert got["span_class"].tolist() == [1, 1, 2, 2, 2, 2, 0]                               # unset | number ... unset | unparsable: the larger, 2
    assert got["span_begin"].tolist() == [0, 3, 0, 2, 0, 0, 10] and got["span_end"].tolist() == [7, 0, 9, 0, 0, 4, 30] and got["span_duration"].tolist() == [0] * 6 + [20]
    t = got["totals"]
    assert t["out_of_range"] == 0 and (t["durations"]["numbers"], t["durations"]["unset"], t["durations"]["not_numbers"]) == (1, 2, 4)
    assert [s["lines"] for s in got["key_span_stats"]] == [1] * 7 and got["key_span_stats"][6]["sum"] == 20 and got["key_span_stats"][0]["min"] is None
    # the END part has no number group: every span is class 1 and keeps its begin's time; then neither part has one
    got = check(gorp, *roles_batch(names([0, 0, 1, 1]), "BEBE", [5, 9, 6, 8]), [(0, 0, 1, "begin"), (1, 0, None, "end")])
    assert got["span_class"].tolist() == [1, 1] and got["span_begin"].tolist() == [5, 6] and got["span_end"].tolist() == [0, 0]
    got = check(gorp, *roles_batch(names([0, 0, 1, 1, 1]), "BEBEB", [5, 9, 6, 8, 9]), [(0, 0, None, "begin"), (1, 0, None, "end")])
    assert got["span_class"].tolist() == [1, 1] and got["totals"]["durations"]["unset"] == 2 and got["totals"]["left_open"] == 1 and got["span_duration"].tolist() == [0, 0]


def test_iso8601_begins_and_clf_ends_in_the_formats_unit():
    gorp = trivial_handle(2, tag="iso-clf")
    gorp.set_number_format(0, 1, "iso8601", 3)
    gorp.set_number_format(1, 1, "clf", 3)
    formats = {(0, 1): ("iso8601", 3), (1, 1): ("clf", 3)}
    keys = [b"r1", b"r2", b"r1", b"r2", b"r3", b"r3", b"r4", b"r4"]
    times = [b"2026-10-11T20:14:15.250Z", b"2026-10-11T22:14:15+02:00", b"11/Oct/2026:22:14:16 +0200", b"11/Oct/2026:20:14:14 +0000",
             b"2026-10-11T20:14:15.250Z", b"yesterday", b"11/Oct/2026:22:14:15 +0200", b"11/Oct/2026:22:14:16 +0200"]
    got = check(gorp, *roles_batch(keys, "BBEEBEBE", times), SP, formats=formats)
    assert got["span_key"].tolist() == [0, 1, 2, 3] and got["span_class"].tolist() == [0, 0, 2, 2]
    assert got["span_duration"].tolist() == [750, -1000, 0, 0]                               # milliseconds: the formats' unit
    assert got["span_begin"].tolist()[0] == 1791749655250 and got["span_end"].tolist()[0] == 1791749656000


@pytest.mark.parametrize("name", sorted(SUM_SEQUENCES))
def test_128_bit_sums_of_durations_per_key(name):
    gorp = trivial_handle(2)
    values = [v for count, v in SUM_SEQUENCES[name] for _ in range(count)]
    assert len(values) == 70000
    rng = np.random.default_rng(3)
    rng.shuffle(values)
    which = rng.integers(0, 3, len(values))
    keys = [k for j in which for k in (b"k%d" % j, b"k%d" % j)]
    times = [t for v in values for t in (0, v)]                                               # begin 0, end v: the duration is v
    got = check(gorp, *roles_batch(keys, "BE" * len(values), times), SP, hooks=False)
    t = got["totals"]
    assert t["n_spans"] == 70000 and t["durations"]["sum"] == sum(values) and sum(s["sum"] for s in got["key_span_stats"]) == sum(values)
    assert any(not INT64_MIN <= s["sum"] <= INT64_MAX for s in got["key_span_stats"]) and t["durations"]["numbers"] == 70000


# ---------------------------------------------------------------------------
# 4. classes, parts, terms
# ---------------------------------------------------------------------------
def mixed_batch(n=900, seed=5, **kw):
    rng = np.random.default_rng(seed)
    times = (np.sort(rng.integers(0, 5000, n)) + rng.integers(-40, 40, n)).tolist()
    values = rng.integers(-500, 900, n).tolist()
    keys = names(rng.integers(0, 9, n))
    for i in rng.integers(0, n, 25):
        times[i] = [None, b"-", b"12x"][i % 3]
    for i in rng.integers(0, n, 25):
        values[i] = [None, b"", b"1e3"][i % 3]
    for i in rng.integers(0, n, 15):
        keys[i] = [None, b""][i % 2]
    ids = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n))
    return batch(keys, times, values, lengths=rng.integers(0, 30, n), ids=ids, **kw)


def test_two_begin_extractions_one_end_extraction_unmatched_lines_unset_keys_and_terms():
    gorp = trivial_handle(3)
    parts = [(0, 0, 1, "begin", 2), (1, 0, 1, "end", 2), (2, 0, 1, "begin", 2)]
    keys = [b"x", b"x", b"y", b"x", None, b"y", b"y", b"z", b"x", b"y", b"z"]
    ids = [0, 1, 2, 2, 0, 1, 0, 1, -1, 1, 2]
    data, offsets, ids, caps = batch(keys, [5, 8, 1, 9, 7, 4, 6, 8, 5, 9, 3], values=[1, 2, 3, 4, 5, 6, 7, None, 9, b"q", 11], lengths=[9] * 11, ids=ids)
    got = check(gorp, data, offsets, ids, caps, parts)
    t = got["totals"]
    assert (t["lines"], t["keyed"], t["unset"], t["begins"], t["ends"]) == (10, 9, 1, 5, 4)
    # x: B0 E1 B3 -> a span and an open begin; y: B2 E5 B6 E9 -> two spans, begun by extraction 2 and by extraction 0; z: E7 B10
    assert got["keys"] == [b"x", b"y", b"z"] and got["line_state"].tolist() == [1, 2, 1, 4, 0, 2, 1, 5, 0, 2, 4]
    assert got["span_begin_line"].tolist() == [0, 2, 6] and got["span_duration"].tolist() == [3, 3, 3] and got["key_open_line"].tolist() == [3, NONE, 10]
    # a term on the END extraction that removes some ends turns their begins into left-open or superseded ones
    base = check(trivial_handle(2), *mixed_batch(), SPV)
    less = check(trivial_handle(2), *mixed_batch(), SPV, where=[(1, 2, "<", 200)])
    a, b = base["totals"], less["totals"]
    assert b["ends"] < a["ends"] and b["begins"] == a["begins"] and b["n_spans"] < a["n_spans"] and b["superseded"] + b["left_open"] > a["superseded"] + a["left_open"]
    assert a["unset"] > 0 and a["durations"]["unset"] > 0 and a["durations"]["not_numbers"] > 0 and a["n_spans"] > 100


def test_no_lines_no_parts_and_keyed_lines_of_a_single_role():
    gorp = trivial_handle(2)
    data, offsets, ids, caps = roles_batch(names([0, 1, 0]), "BEE")
    got = check(gorp, data, offsets, ids, caps, [])                                           # no part at all
    assert got["totals"]["n_spans"] == 0 and got["key_span_begin"].tolist() == [0] and set(got["line_span"].tolist()) == {NONE} and got["line_state"].tolist() == [0, 0, 0]
    assert len(got["key_open_line"]) == 0 and got["key_span_stats"] == []
    got = check(gorp, *batch([], []), SP)                                                     # no line at all
    assert got["totals"]["n_spans"] == 0 and len(got["line_span"]) == 0 and len(got["line_state"]) == 0 and got["key_span_begin"].tolist() == [0]
    assert [got["totals"][name] for name in SPAN_TOTALS] == [0] * 7 and got["totals"]["durations"]["lines"] == 0
    got = check(gorp, *roles_batch([None, None], "BE"), SP)                                   # counted lines, none of them keyed
    assert got["totals"]["lines"] == 2 and got["totals"]["keyed"] == 0 and got["key_span_begin"].tolist() == [0] and got["line_state"].tolist() == [0, 0]
    got = check(gorp, data, offsets, ids, caps, [(1, 0, 1, "end")])                           # the END part alone: keyed lines of a single role
    assert got["totals"]["ends"] == 2 and got["totals"]["orphan_ends"] == 2 and got["line_state"].tolist() == [0, 5, 5]
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, "begin")])
    assert got["totals"]["begins"] == 1 and got["totals"]["left_open"] == 1 and got["key_open_line"].tolist() == [0]
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, "end"), (1, 0, 1, "begin")])       # the roles the other way round: E B B
    assert got["line_state"].tolist() == [5, 4, 4] and got["keys"] == [b"k0", b"k1"] and got["key_open_line"].tolist() == [2, 1]


# ---------------------------------------------------------------------------
# 5. every way the batch is read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [np.uint16, np.uint8])
def test_compact_result_rows(rows):
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch()
    base = check(gorp, data, offsets, ids, caps, SPV, hooks=False)
    got = check(gorp, data, offsets, pack(ids, caps, rows), None, SPV)
    assert got["totals"] == base["totals"] and got["key_span_stats"] == base["key_span_stats"] and all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)


def test_offsets64_utf16_and_utf8_bytes():
    gorp = trivial_handle(2)
    base = check(gorp, *mixed_batch(), SPV)
    for kw, utf8 in ((dict(offsets_dtype=np.uint64), None), (dict(dtype=np.uint16), None), (dict(dtype=np.uint16, offsets_dtype=np.uint64), None), ({}, "bytes")):
        got = check(gorp, *mixed_batch(**kw), SPV, utf8=utf8)
        assert {k: got["totals"][k] for k in SPAN_TOTALS + ("durations",)} == {k: base["totals"][k] for k in SPAN_TOTALS + ("durations",)}
        assert got["key_span_stats"] == base["key_span_stats"] and all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)


# ---------------------------------------------------------------------------
# 6. the calling forms
# ---------------------------------------------------------------------------
OUTS = ("span_key", "span_begin_line", "span_end_line", "span_begin", "span_end", "span_duration", "span_class", "key_span_begin", "key_span_stats", "key_open_line",
        "line_span", "line_state")
KEY_OUTS = ("key_units", "key_offsets", "key_first_line", "key_lines", "key_stats", "line_key")


def raw_call(gorp, data, offsets, ids, caps, parts, max_spans, max_keys=64, want=OUTS + KEY_OUTS, poison=0xAB, spans=True):
    """gx_group_spans itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p, numbers, roles = gorp.span_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n = len(offsets) - 1
    ms = max_spans
    sizes = {"span_key": 4 * (ms + 8), "span_begin_line": 4 * (ms + 8), "span_end_line": 4 * (ms + 8), "span_begin": 8 * (ms + 8), "span_end": 8 * (ms + 8),
             "span_duration": 8 * (ms + 8), "span_class": ms + 8, "key_span_begin": 8 * (max_keys + 9), "key_span_stats": 64 * (max_keys + 8),
             "key_open_line": 4 * (max_keys + 8), "line_span": 4 * (n + 8), "line_state": n + 8, "key_units": 4096, "key_offsets": 4 * (max_keys + 9),
             "key_first_line": 4 * (max_keys + 8), "key_lines": 8 * (max_keys + 8), "key_stats": 64 * (max_keys + 8), "line_key": 4 * (n + 8)}
    arrays = {name: np.full(size, poison, np.uint8) for name, size in sizes.items()}
    ptr = lambda name: arrays[name].ctypes.data if name in want and (p.has_values or name != "key_stats") else None
    keys = N.gx_group_out(ptr("key_units"), 4096, ptr("key_offsets"), ptr("key_first_line"), ptr("key_lines"), ptr("key_stats"), ptr("line_key"), max_keys)
    out = N.gx_spans_out(*[ptr(name) for name in OUTS], max_spans)
    totals = N.gx_spans_totals()
    rc = N.lib().gx_group_spans(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, numbers, roles, None, 0, 0,
                                C.byref(keys), C.byref(out) if spans else None, C.byref(totals), C.byref(o))
    return rc, Gorp._spans_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a == poison).all() for a in arrays.values())


def test_capacities_poisoned_outputs_the_size_query_and_spans_null():
    gorp = trivial_handle(2)
    # 3 keys x 11 spans, each B E, the pairs of the keys interleaved; then an open begin and an orphan end
    rng = np.random.default_rng(33)
    k = np.repeat(np.concatenate([np.arange(3), rng.permutation(np.repeat(np.arange(3), 10))]), 2)       # (key numbers by first appearance: 0, 1, 2)
    data, offsets, ids, caps = roles_batch(names(k) + [b"k0", b"k1"], "BE" * 33 + "BE", (np.arange(68) * 10).tolist())
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 33, max_keys=3)                          # exactly sufficient
    assert rc == N.GX_OK and [totals[name] for name in SPAN_TOTALS] == [33, 34, 34, 0, 1, 1, 0] and identities(totals)
    assert arrays["span_key"].view(np.uint32)[:33].tolist() == [0] * 11 + [1] * 11 + [2] * 11 and (arrays["span_key"][4 * 33:] == 0xAB).all()
    assert arrays["span_duration"].view(np.int64)[:33].tolist() == [10] * 33 and (arrays["span_duration"][8 * 33:] == 0xAB).all()
    assert (arrays["span_class"][:33] == 0).all() and (arrays["span_class"][33:] == 0xAB).all() and (arrays["span_begin"][8 * 33:] == 0xAB).all()
    assert (arrays["span_begin_line"][4 * 33:] == 0xAB).all() and (arrays["span_end_line"][4 * 33:] == 0xAB).all() and (arrays["span_end"][8 * 33:] == 0xAB).all()
    assert arrays["key_span_begin"].view(np.uint64)[:4].tolist() == [0, 11, 22, 33] and (arrays["key_span_begin"][8 * 4:] == 0xAB).all()
    assert arrays["key_open_line"].view(np.uint32)[:3].tolist() == [66, NONE, NONE] and (arrays["key_open_line"][4 * 3:] == 0xAB).all()
    assert arrays["key_span_stats"].view(np.uint64)[:24].reshape(3, 8)[:, 0].tolist() == [11, 11, 11] and (arrays["key_span_stats"][64 * 3:] == 0xAB).all()
    assert (arrays["line_span"][4 * 68:] == 0xAB).all() and (arrays["line_state"][68:] == 0xAB).all() and arrays["line_state"][:68].tolist() == [1, 2] * 33 + [4, 5]
    fit = totals
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 32, max_keys=3)                          # one span too few: nothing is written
    assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_spans" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 32, max_keys=3, want=("line_span", "line_state", "key_span_begin", "key_open_line") + KEY_OUTS)
    assert rc == N.GX_OK and totals == fit                                                                     # ... max_spans binds the per-span arrays alone
    for name in ("key_span_begin", "key_open_line", "key_span_stats"):                                         # these are sized by max_keys
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 33, max_keys=2, want=(name,))
        assert rc == N.GX_E_LIMIT and totals == fit and untouched(arrays) and "max_keys" in N.last_error(), name
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 0, want=())                              # the size query writes nothing
    assert rc == N.GX_OK and totals == fit and untouched(arrays)
    # the key table's own overflow: the span totals are zero
    rc, totals, arrays = raw_call(gorp, *roles_batch(names(np.arange(65)), "B" * 65), SP, 1024, max_keys=32)
    assert rc == N.GX_E_LIMIT and not totals["group"]["exact"] and totals["group"]["n_keys"] == 65 and untouched(arrays)
    assert [totals[name] for name in SPAN_TOTALS] == [0] * 7 and totals["durations"]["lines"] == 0
    # spans == NULL: the call is gx_group_lines bit for bit, the span totals zero
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, SP, 33, spans=False)
    assert rc == N.GX_OK and totals["group"]["n_keys"] == 3 and [totals[name] for name in SPAN_TOTALS] == [0] * 7
    keys = gorp.group_lines(data, offsets, ids, caps, gorp.span_parts(SP)[0])
    assert totals["group"] == keys["totals"] and arrays["line_key"][:4 * 68].tobytes() == keys["line_key"].tobytes()
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
    host = check(gorp, data, offsets, ids, caps, SPV)
    t = host["totals"]
    s, k, n = t["n_spans"], t["n_keys"], len(ids)
    assert s > 500
    dev = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    d_data, d_off, d_ids, d_caps = dev(data), dev(offsets), dev(ids), dev(caps)
    streams = [new_stream(), new_stream()]
    torch.cuda.synchronize()
    args = (d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), SPV)
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_spans_device(*args, max_keys=16, stream=streams[0].cuda_stream)                    # the size query: every output NULL
    assert rc == N.GX_OK and totals == t
    runs = []
    mk = lambda count, dtype: torch.full((count + 4,), 0x5A, dtype=dtype, device="cuda")
    for stream in streams:                                                                     # the second call right behind the first, on another stream
        out = {"span_key": mk(s, torch.int32), "span_begin_line": mk(s, torch.int32), "span_end_line": mk(s, torch.int32), "span_begin": mk(s, torch.int64),
               "span_end": mk(s, torch.int64), "span_duration": mk(s, torch.int64), "span_class": mk(s, torch.uint8), "key_span_begin": mk(k + 1, torch.int64),
               "key_span_stats": mk(8 * k, torch.int64), "key_open_line": mk(k, torch.int32), "line_span": mk(n, torch.int32), "line_state": mk(n, torch.uint8),
               "line_key": mk(n, torch.int32), "key_lines": mk(k, torch.int64)}
        with torch.cuda.stream(stream):
            rc, totals = gorp.group_spans_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k, max_spans=s,
                                                 stream=stream.cuda_stream, **{name + "_ptr": out[name].data_ptr() for name in OUTS})
        assert rc == N.GX_OK and totals == t
        runs.append(out)
    for stream in streams:
        stream.synchronize()                                                                   # the outputs are read after a stream wait
    x, y = [{name: a.cpu().numpy() for name, a in out.items()} for out in runs]
    assert all(x[name].tobytes() == y[name].tobytes() for name in x)
    for name, dtype in SPAN_FIELDS:
        c = len(host[name])
        assert x[name][:c].view(dtype).tolist() == host[name].tolist() and (x[name][c:] == 0x5A).all(), name
    assert x["line_key"][:n].view(np.uint32).tolist() == host["line_key"].tolist() and x["key_lines"][:k].tolist() == host["lines"].tolist()
    stats = x["key_span_stats"][:8 * k].reshape(k, 8)
    assert (x["key_span_stats"][8 * k:] == 0x5A).all()
    for j, st in enumerate(host["key_span_stats"]):
        assert stats[j, :4].tolist() == [st["lines"], st["numbers"], st["unset"], st["not_numbers"]]
        assert st["numbers"] == 0 or (int(stats[j, 4]), int(stats[j, 5])) == (st["min"], st["max"])
        assert (int(stats[j, 7]) << 64) + (int(stats[j, 6]) & (2 ** 64 - 1)) == st["sum"]
    # a capacity too small with device pointers: nothing is written, the key outputs included
    out = {"span_key": mk(s, torch.int32), "line_key": mk(n, torch.int32), "key_lines": mk(k, torch.int64), "line_state": mk(n, torch.uint8)}
    with torch.cuda.stream(streams[0]):
        rc, totals = gorp.group_spans_device(*args, key_lines_ptr=out["key_lines"].data_ptr(), line_key_ptr=out["line_key"].data_ptr(), max_keys=k,
                                             span_key_ptr=out["span_key"].data_ptr(), line_state_ptr=out["line_state"].data_ptr(), max_spans=s - 1,
                                             stream=streams[0].cuda_stream)
    streams[0].synchronize()
    assert rc == N.GX_E_LIMIT and totals == t and all((a.cpu().numpy() == 0x5A).all() for a in out.values())


# ---------------------------------------------------------------------------
# 7. end to end: a start rule and an end rule that share an id, extracted on the device, and the same from raw text
# ---------------------------------------------------------------------------
def test_a_start_rule_and_an_end_rule_end_to_end_and_from_raw_text():
    stamp = [["text", "["], ["extractor", "ts", [["pattern", "[\\w:.-]+"]]], ["text", "] "]]
    gorp = Gorp.construct([FlattenedExtraction("RequestStart", stamp + [["text", "start "], ["extractor", "id", [["pattern", "\\w+"]]]]),
                           FlattenedExtraction("RequestEnd", stamp + [["text", "end "], ["extractor", "id", [["pattern", "\\w+"]]]])])
    for k in range(2):
        gorp.set_number_format(k, "ts", "iso8601", 3)
    rng = np.random.default_rng(12)
    lines = []
    for i in range(600):
        ms = 1000 * i + int(rng.integers(0, 999))
        ts = b"2026-01-03T%02d:%02d:%02d.%03dZ" % (ms // 3_600_000, ms // 60_000 % 60, ms // 1000 % 60, ms % 1000)
        kind = int(rng.integers(0, 10))
        lines.append(b"noise %d" % i if kind == 0 else b"[%s] %s req%d" % (b"soon" if kind == 1 else ts, b"start" if kind < 6 else b"end", int(rng.integers(0, 40))))
    data = np.frombuffer(b"".join(lines), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids == 0).sum() > 200 and (ids == 1).sum() > 150 and (ids < 0).sum() > 30
    parts = [("RequestStart", "id", "ts", "begin"), ("RequestEnd", "id", "ts", "end")]
    formats = {(k, gorp._extraction_and_group(k, "ts")[1]): ("iso8601", 3) for k in range(2)}
    got = check(gorp, data, offsets, ids, caps, parts, formats=formats)
    t = got["totals"]
    assert t["n_spans"] > 100 and t["superseded"] > 20 and t["left_open"] > 3 and t["orphan_ends"] > 10 and t["durations"]["not_numbers"] > 5 and t["n_keys"] == 40
    assert t["durations"]["min"] > 0 and t["durations"]["numbers"] > 80                                        # the log's clock only moves forward
    # the whole-file form: raw text in, the same keys and spans out, counts and n_lines as text_group_lines gives them
    raw = b"\n".join(lines) + b"\n"
    text, counts, n_lines = gorp.text_group_spans(raw, parts)
    keys, kcounts, kn = gorp.text_group_lines(raw, gorp.span_parts(parts)[0])
    assert n_lines == kn == len(ids) and counts.tolist() == kcounts.tolist() and counts[:2].tolist() == [int((ids == k).sum()) for k in range(2)]
    assert text["totals"] == got["totals"] and text["key_span_stats"] == got["key_span_stats"] and text["keys"] == got["keys"] == keys["keys"]
    assert all(text[f].tobytes() == got[f].tobytes() for f in FIELDS + KEY_FIELDS) and text["totals"]["group"] == keys["totals"]


# ---------------------------------------------------------------------------
# 8. one large shape
# ---------------------------------------------------------------------------
def test_three_hundred_thousand_lines_against_numpy():
    gorp = trivial_handle(2)
    n = 300_000
    key, role, t, matched = draw(n, seed=20)
    want = np_spans(key, role, t, matched)
    counts = np.bincount(want["line_state"], minlength=6)
    assert (counts[1:] > 2000).all() and counts[1] == counts[2]                                # all five entry states occur in the thousands
    data, offsets, ids, caps = wide_batch(key, role, t, matched)
    got = gorp.group_spans(data, offsets, ids, caps, SP, max_keys=8192, keys="csr")
    tt = got["totals"]
    assert identities(tt) and tt["keyed"] == tt["lines"] == int(matched.sum()) and tt["n_keys"] == 4000
    assert [tt[name] for name in SPAN_TOTALS] == [int(counts[2]), int(counts[1] + counts[3] + counts[4]), int(counts[2] + counts[5]), int(counts[3]), int(counts[4]),
                                                  int(counts[5]), 0]
    for name, dtype in SPAN_FIELDS:
        assert got[name].dtype == want[name].dtype == dtype and np.array_equal(got[name], want[name]), name
    d = want["span_duration"]
    assert tt["durations"] == {"lines": len(d), "numbers": len(d), "unset": 0, "not_numbers": 0, "min": int(d.min()), "max": int(d.max()), "sum": int(d.sum())}
    per_key = np.zeros(tt["n_keys"], np.int64)
    np.add.at(per_key, want["span_key"], d)
    assert [s["sum"] for s in got["key_span_stats"]] == per_key.tolist() and [s["lines"] for s in got["key_span_stats"]] == np.diff(want["key_span_begin"].astype(np.int64)).tolist()
