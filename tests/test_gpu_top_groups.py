"""GPU tests of gx_top_groups / gx_text_top_groups: the keys of a batch ranked by their lines or by the numbers their lines captured.

Expected values come from tests/top_groups_oracle.py -- group_oracle.group_lines for the keys and their stats, a rank value per key as a
Python int, sorted() by (-value, key number) -- and everything is compared bit for bit.  Most batches are fabricated against handles of K
identical, trivial extractions with two groups: a line is "key value", its capture row (0, |key|, |key| + 1, |line|), its id chosen
here; the end-to-end cases take ids and rows from gx_extract_batch.  The large shape is compared with a numpy restatement (np.lexsort),
which tests/test_top_groups_host.py compares with the oracle on smaller draws of the same generator."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, split_lines
from group_oracle import decode_parts
from top_groups_oracle import RANK_BY, TOP_GROUPS_MAX, np_top, same, skewed_draw, top_groups
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_top_groups.hip")).read()
SHARE = 256 * int(re.search(r"TG_SWEEP_KEYS = (\d+)", SRC).group(1))     # keys a histogram workgroup takes per trip: up to it ONE launch selects, above it the slab has two entries
SCAN_BLOCK = 2048                                                        # gx_scan.hpp: SCAN_THREADS x SCAN_ITEMS
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
TIME = "timeTakenInMsec"
BY_VERB = [("PutRequest", "verb", TIME), ("GetRequest", "verb", TIME), ("OtherRequest", "verb", TIME)]
BY_PATH = [("PutRequest", "path", TIME), ("GetRequest", "path", TIME), ("OtherRequest", "path", TIME)]
KV = [(0, 0, 1)]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, n, by="lines", largest=True, where=None, utf8=None, **kw):
    """top_groups against the restatement, every field, and the invariants; returns what the call returned."""
    p = gorp.group_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = top_groups(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions, n, by, largest)
    got = gorp.top_groups(data, offsets, ids, caps, p, n, by=by, largest=largest, where=terms, utf8=utf8, keys="csr", line_rank=True, **kw)
    same(got, want, n, largest, data.dtype)
    return got


def plain(res):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}


_handles = {}


def trivial_handle(K, groups=2):
    """K identical extractions `a(.*)(.*)`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups].num_extractions == K and _handles[K, groups].max_groups == groups
    return _handles[K, groups]


def kv_batch(keys, values, ids=None, dtype=np.uint8, offsets_dtype=np.uint32):
    """a line is "key value": group 0 the key, group 1 the value (bytes, or sequences of code units)"""
    lens = np.array([len(k) + 1 + len(v) for k, v in zip(keys, values)], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(offsets_dtype)
    data = np.fromiter((u for k, v in zip(keys, values) for part in (k, (0x20,), v) for u in part), dtype=dtype, count=int(lens.sum()))
    klen = np.array([len(k) for k in keys], np.int32)
    caps = np.stack([np.zeros(len(klen), np.int32), klen, klen + 1, lens.astype(np.int32)], axis=1).reshape(len(klen), 4)
    return data, offsets, np.zeros(len(klen), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def numbered(key_numbers, numbers, ids=None, **kw):
    """kv_batch of key names (spelled k<name>) and int values"""
    return kv_batch([b"k%d" % k for k in key_numbers], [b"%d" % v for v in numbers], ids, **kw)


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


FIELDS = ("units", "offsets", "number", "first", "lines", "stats", "line_rank")


def raw_call(gorp, data, offsets, ids, caps, parts, n_wanted, by="lines", cap_keys=0, units_cap=0, max_keys=0, want=FIELDS, flags=0, poison=0xAB, **kw):
    """gx_top_groups itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.group_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"units": np.zeros(units_cap + 8, data.dtype), "offsets": np.zeros(cap_keys + 1 + 8, offsets.dtype), "number": np.zeros(cap_keys + 8, np.uint32),
              "first": np.zeros(cap_keys + 8, np.uint32), "lines": np.zeros(cap_keys + 8, np.uint64), "stats": np.zeros((cap_keys + 8) * 64, np.uint8),
              "line_rank": np.zeros(n + 8, np.uint32)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_top_groups_out(ptr("units"), units_cap, ptr("offsets"), ptr("number"), ptr("first"), ptr("lines"), ptr("stats") if p.has_values else None,
                              ptr("line_rank"), cap_keys)
    totals = N.gx_top_groups_totals()
    rc = N.lib().gx_top_groups(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
                               None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, Gorp.RANK_BY[by], n_wanted, max_keys, flags,
                               C.byref(out) if want else None, C.byref(totals), C.byref(o))
    return rc, Gorp._top_groups_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


# ---------------------------------------------------------------------------
# the README definition, extracted for real
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def readme():
    gorp = Gorp.construct(W.readme3_definition())
    n = 1500
    t_data, _, cat = W.readme3_lines(n, seed=5)
    data = t_data.numpy().copy()
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(ids, cat.numpy().astype(np.int32))
    return gorp, data, offsets, ids, caps


@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_readme_definition_in_every_row_format_and_offset_width(readme, fmt, offsets_dtype):
    gorp, data, offsets, ids, caps = readme
    offsets = offsets.astype(offsets_dtype)
    if fmt == "int32":
        id_col, rows = ids, caps
    else:
        id_col, rows = gorp.extract_batch(data, offsets, compact=1 if fmt == "u16" else 2)[0], None
    # the verbs by their lines and by the sum of timeTakenInMsec; the paths that took the longest, and the ones that never did
    by_lines = check(gorp, data, offsets, id_col, rows, BY_VERB, 10)
    assert by_lines["totals"]["n_top"] == 6 and by_lines["key_offsets"].dtype == offsets_dtype
    listed = gorp.top_groups(data, offsets, id_col, rows, BY_VERB, 3, by="sum")
    whole = gorp.group_lines(data, offsets, id_col, rows, BY_VERB)
    best = sorted(range(6), key=lambda j: (-whole["stats"][j]["sum"], j))[:3]
    assert listed["keys"] == [whole["keys"][j] for j in best] and listed["key_number"].tolist() == best and "line_rank" not in listed
    check(gorp, data, offsets, id_col, rows, BY_PATH, 10, by="max")
    check(gorp, data, offsets, id_col, rows, BY_PATH, 10, by="max", largest=False)
    check(gorp, data, offsets, id_col, rows, BY_PATH, 25, by="numbers", where=[("GetRequest", TIME, ">=", 500), ("OtherRequest", "verb", "!=", "POST")])


# ---------------------------------------------------------------------------
# key counts at the edges of a wave, a workgroup, a histogram workgroup's share
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 63, 64, 65, 255, 256, 257, SHARE - 1, SHARE, SHARE + 1, 2 * SHARE + 3])
def test_key_counts_at_the_edges(n_keys):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n_keys)
    names = np.concatenate([rng.permutation(n_keys), rng.integers(0, n_keys, n_keys // 2)])        # every key once, half of them again
    values = rng.integers(-500, 500, len(names))
    data, offsets, ids, caps = numbered(names, values)
    for by, largest, n in (("lines", True, 5), ("sum", True, n_keys // 2 + 1), ("min", False, 64), ("max", True, n_keys)):
        got = check(gorp, data, offsets, ids, caps, KV, min(n, TOP_GROUPS_MAX), by=by, largest=largest, max_keys=n_keys)
        assert got["totals"]["candidates"] == n_keys
    # through the slots instead of the flagged first lines -- a table much smaller than the batch: the same rule
    if n_keys <= 65:
        slots = max(64, 1 << (2 * n_keys - 1).bit_length())
        reps = 16 * slots // len(names) + 1
        assert 16 * slots < reps * len(names)           # (gx_top_groups.hip: top_groups_by_slots)
        d2, o2, i2, c2 = numbered(np.tile(names, reps), np.tile(values, reps))
        got = check(gorp, d2, o2, i2, c2, KV, 7, by="sum", max_keys=n_keys)
        assert got["totals"]["group"]["n_keys"] == n_keys and got["lines"].sum() <= reps * len(names)


def test_one_large_skewed_batch_against_numpy():
    gorp = trivial_handle(1)
    names, values = skewed_draw(200000, 100000, seed=1)
    data, offsets, ids, caps = numbered(names, values)
    n = len(names)
    for by, largest, n_wanted in (("lines", True, 100), ("lines", False, TOP_GROUPS_MAX), ("sum", True, TOP_GROUPS_MAX), ("max", False, 1000), ("min", True, 10),
                                  ("numbers", True, 3000)):
        order, v, n_keys, ties_left = np_top(names, values, n_wanted, by, largest)
        assert 60000 < n_keys < 80000 and n_keys > TOP_GROUPS_MAX
        got = gorp.top_groups(data, offsets, ids, caps, KV, n_wanted, by=by, largest=largest, keys="csr", max_keys=n, line_rank=(by == "sum"))
        t = got["totals"]
        assert t["group"]["n_keys"] == t["candidates"] == n_keys and t["n_top"] == len(order) == n_wanted and t["ties_left"] == ties_left and t["last"] == int(v[-1])
        assert np.array_equal(got["key_number"], order)
        rank_value = {"lines": got["lines"].astype(np.int64), "numbers": np.array([s["numbers"] for s in got["stats"]]),
                      "sum": np.array([s["sum"] for s in got["stats"]]), "max": np.array([s["max"] for s in got["stats"]]),
                      "min": np.array([s["min"] for s in got["stats"]])}[by]
        assert np.array_equal(rank_value, v)
        # the keys' text: k<name> of the key's first line
        koff = got["key_offsets"].astype(np.int64)
        assert [bytes(got["key_units"][koff[r]:koff[r + 1]]) for r in (0, n_wanted // 2, n_wanted - 1)] == [b"k%d" % names[got["first_line"][r]] for r in (0, n_wanted // 2, n_wanted - 1)]
        if by == "sum":
            _, first, inverse = np.unique(names, return_index=True, return_inverse=True)
            number = np.empty(len(first), np.int64)
            number[np.argsort(first)] = np.arange(len(first))
            rank_of = np.full(n_keys, 0xFFFFFFFF, np.uint32)
            rank_of[order] = np.arange(n_wanted)
            assert np.array_equal(got["line_rank"], rank_of[number[inverse]])


# ---------------------------------------------------------------------------
# ties at the cut
# ---------------------------------------------------------------------------
def test_all_keys_tie_and_the_first_key_numbers_win():
    gorp = trivial_handle(1)
    n_keys = 700
    data, offsets, ids, caps = numbered(np.arange(n_keys)[::-1], np.full(n_keys, 42))
    for by in RANK_BY:
        for largest in (True, False):
            for n in (1, 100, n_keys, TOP_GROUPS_MAX):
                got = check(gorp, data, offsets, ids, caps, KV, n, by=by, largest=largest, max_keys=n_keys)
                k = min(n, n_keys)
                assert got["key_number"].tolist() == list(range(k)) and got["totals"]["ties_left"] == n_keys - k


@pytest.mark.parametrize("largest", [True, False])
def test_a_tie_run_across_a_wave_a_workgroup_and_a_scan_block_cut_in_its_middle(largest):
    gorp = trivial_handle(1)
    n_keys = SCAN_BLOCK + 700
    better, worse, tie = (9, 1, 5) if largest else (1, 9, 5)
    values = np.full(n_keys, tie)
    values[:30] = better                              # thirty keys ahead of the run, which starts inside the first wave ...
    values[40:50] = worse                             # ... is interrupted there ...
    values[SCAN_BLOCK + 100:] = worse                 # ... and ends behind the first scan block
    run = int((values == tie).sum())
    data, offsets, ids, caps = numbered(np.arange(n_keys), values)
    for taken in (1, 20, 64 - 30 - 10 + 1, 300, SCAN_BLOCK - 40 - 1, SCAN_BLOCK - 40, SCAN_BLOCK - 40 + 1, run - 1, run):
        got = check(gorp, data, offsets, ids, caps, KV, 30 + taken, by="max", largest=largest, max_keys=n_keys)
        assert got["totals"]["ties_left"] == run - taken and got["totals"]["last"] == tie
        assert got["key_number"][:30].tolist() == list(range(30)) and (np.diff(got["key_number"][30:].astype(np.int64)) > 0).all()


# ---------------------------------------------------------------------------
# every rank_by, both directions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("by", RANK_BY)
def test_every_rank_value_with_negatives_keys_without_numbers_and_sums_beyond_int64(by, largest):
    gorp = trivial_handle(3)
    rng = random.Random(7)
    keys, values, ids = [], [], []
    def add(key, value, k=0):
        keys.append(key); values.append(value); ids.append(k)
    for j in range(40):                               # negative and positive numbers, several lines per key
        for _ in range(rng.randrange(1, 5)):
            add(b"n%d" % j, b"%d" % rng.randrange(-1000, 1000))
    for j in range(10):                               # keys without numbers: not a number, and an unset value (below)
        add(b"x%d" % j, b"abc")
        add(b"u%d" % j, b"0")
    for j, (v, times) in enumerate([(INT64_MAX, 2), (INT64_MAX, 3), (INT64_MAX, 4), (INT64_MIN, 2), (INT64_MIN, 3), (INT64_MIN, 4), (INT64_MAX, 4)]):
        for _ in range(times):                        # sums that differ only in sum_hi
            add(b"big%d" % j, b"%d" % v)
    for j in range(12):                               # extraction 1 only counts: its lines add to `lines` alone, in the same key space
        add(b"n%d" % j, b"5", 1)
        add(b"only%d" % j, b"5", 1)
    add(b"other", b"1", 2)                            # extraction 2 has no part
    data, offsets, ids, caps = kv_batch(keys, values, ids)
    for i, k in enumerate(keys):
        if k.startswith(b"u"):
            caps[i, 2:] = -1                          # the value group is unset
    parts = [(0, 0, 1), (1, 0)]
    for n in (0, 1, 17, 60, 200):
        got = check(gorp, data, offsets, ids, caps, parts, n, by=by, largest=largest)
    t = got["totals"]
    assert t["group"]["n_keys"] == 40 + 20 + 7 + 12 and t["candidates"] == (t["group"]["n_keys"] if by in ("lines", "numbers") else 47)
    if by == "sum":
        assert (got["stats"][0]["sum"] == 4 * INT64_MAX and got["key_number"][:2].tolist() == [62, 66]) if largest else got["stats"][0]["sum"] == 4 * INT64_MIN


# ---------------------------------------------------------------------------
# n_wanted
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [300, TOP_GROUPS_MAX])
def test_everything_wanted_is_a_permutation_of_group_lines_rows(n_keys):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n_keys)
    names = np.concatenate([rng.permutation(n_keys), rng.integers(0, n_keys, n_keys)])
    values = rng.integers(-50, 50, len(names))
    data, offsets, ids, caps = numbered(names, values)
    whole = gorp.group_lines(data, offsets, ids, caps, KV, keys="csr", max_keys=n_keys, key_units_cap=8 * n_keys)
    assert whole["totals"]["n_keys"] == n_keys
    for by, largest, n in (("sum", True, TOP_GROUPS_MAX), ("lines", False, n_keys), ("max", True, n_keys)):
        got = gorp.top_groups(data, offsets, ids, caps, KV, n, by=by, largest=largest, keys="csr", max_keys=n_keys, line_rank=True)
        j = got["key_number"]
        assert got["totals"]["n_top"] == n_keys and sorted(j.tolist()) == list(range(n_keys)) and got["totals"]["group"] == whole["totals"]
        assert np.array_equal(got["first_line"], whole["first_line"][j]) and np.array_equal(got["lines"], whole["lines"][j])
        assert got["stats"] == [whole["stats"][x] for x in j]
        wo, go = whole["key_offsets"].astype(np.int64), got["key_offsets"].astype(np.int64)
        assert all(bytes(got["key_units"][go[r]:go[r + 1]]) == bytes(whole["key_units"][wo[x]:wo[x + 1]]) for r, x in enumerate(j.tolist()))
        assert np.array_equal(j[got["line_rank"]], whole["line_key"])
        sign = -1 if largest else 1
        value = [sign * (s["sum"] if by == "sum" else s["max"] if by == "max" else s["lines"]) for s in got["stats"]]
        assert all(a < b for a, b in zip(zip(value, j.tolist()), list(zip(value, j.tolist()))[1:]))
    if n_keys == 300:
        check(gorp, data, offsets, ids, caps, KV, 0, by="sum")
        check(gorp, data, offsets, ids, caps, KV, 1, by="sum")
        check(gorp, data, offsets, ids, caps, KV, TOP_GROUPS_MAX, by="min", largest=False)


def test_no_lines_no_parts_nothing_wanted():
    gorp = trivial_handle(2)
    data, offsets, ids, caps = numbered([1, 2, 1], [5, 6, 7])
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros((0, 4), np.int32))
    for batch, parts in ((empty, KV), ((data, offsets, ids, caps), []), ((data, offsets, ids, caps), [(1, 0, 1)])):
        got = check(gorp, *batch, parts, 5)
        assert got["totals"]["n_top"] == 0 and got["totals"]["last"] is None and got["key_offsets"].tolist() == [0]
        assert (got["line_rank"] == 0xFFFFFFFF).all()
    got = check(gorp, data, offsets, ids, caps, KV, 0, by="sum")
    assert got["totals"]["candidates"] == 2 and got["totals"]["group"]["n_keys"] == 2


# ---------------------------------------------------------------------------
# row formats and batch options
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_compact_rows_and_wide_offsets(dtype):
    gorp = trivial_handle(2)
    rng = np.random.default_rng(3)
    n = 900
    names, values, ids = rng.integers(0, 120, n), rng.integers(-10 ** 5, 10 ** 5, n), rng.integers(-1, 2, n)
    data, offsets, ids, caps = numbered(names, values, ids, offsets_dtype=np.uint64)
    rows = pack(ids, caps, dtype)
    parts = [(0, 0, 1), (1, 0, 1)]
    for by in ("lines", "sum"):
        a = check(gorp, data, offsets, ids, caps, parts, 50, by=by)
        b = check(gorp, data, offsets, rows, None, parts, 50, by=by)
        assert plain(a) == plain(b) and a["key_offsets"].dtype == np.uint64


def test_utf16_units_and_utf8_bytes():
    gorp = trivial_handle(1)
    rng = random.Random(4)
    alphabet = [(0x3B1, 0x62), (0x62,), (0x416, 0x20AC, 0x63), (0xD83D, 0xDE00), (0x100,), (0x1, 0x100)]       # units above 0xFF in the keys
    keys = [rng.choice(alphabet) for _ in range(300)]
    values = [tuple(b"%d" % rng.randrange(-99, 99)) for _ in keys]
    data, offsets, ids, caps = kv_batch(keys, values, dtype=np.uint16)
    for by, largest in (("lines", True), ("sum", False), ("max", True)):
        got = check(gorp, data, offsets, ids, caps, KV, 4, by=by, largest=largest)
        assert got["key_units"].dtype == np.uint16 and got["totals"]["candidates"] == 6
    listed = gorp.top_groups(data, offsets, ids, caps, KV, 6)
    assert sorted(listed["keys"]) == sorted("".join(map(chr, a)) if a != (0xD83D, 0xDE00) else "\U0001F600" for a in alphabet)
    texts = ["café", "caf", "Ж€", "€Ж", "x"]
    keys8 = [rng.choice(texts).encode("utf-8") for _ in range(300)]
    data, offsets, ids, caps = kv_batch(keys8, [b"%d" % rng.randrange(-99, 99) for _ in keys8])
    check(gorp, data, offsets, ids, caps, KV, 3, by="sum", utf8="bytes")
    listed = gorp.top_groups(data, offsets, ids, caps, KV, 5, utf8="bytes")
    assert sorted(listed["keys"]) == sorted(texts) and all(isinstance(k, str) for k in listed["keys"])


def test_terms_remove_lines_and_whole_keys_and_the_weak_hash_changes_nothing():
    gorp = trivial_handle(2)
    rng = np.random.default_rng(8)
    n = 1200
    names, values, ids = rng.integers(0, 200, n), rng.integers(0, 100, n), rng.integers(0, 2, n)
    values[names >= 150] = rng.integers(0, 10, int((names >= 150).sum()))              # these keys lose every line to the term
    data, offsets, ids, caps = numbered(names, values, ids)
    parts = [(0, 0, 1), (1, 0, 1)]
    where = [(0, 1, ">=", 10), (1, 1, ">=", 10)]
    without = check(gorp, data, offsets, ids, caps, parts, 300, by="lines")
    got = check(gorp, data, offsets, ids, caps, parts, 300, by="lines", where=where)
    assert got["totals"]["group"]["n_keys"] < without["totals"]["group"]["n_keys"] and got["totals"]["group"]["lines"] < without["totals"]["group"]["lines"]
    for by, largest in (("sum", True), ("min", False)):
        strong = check(gorp, data, offsets, ids, caps, parts, 40, by=by, largest=largest, where=where)
        weak = check(gorp, data, offsets, ids, caps, parts, 40, by=by, largest=largest, where=where, weak_hash=True)
        assert plain(strong) == plain(weak)


# ---------------------------------------------------------------------------
# the size query, capacities, the overflowed table
# ---------------------------------------------------------------------------
def test_the_size_query_and_every_limit_leave_the_outputs_untouched():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(12)
    names = np.concatenate([np.arange(100), rng.integers(0, 100, 300)])
    data, offsets, ids, caps = numbered(names, rng.integers(-9, 9, 400))
    host = check(gorp, data, offsets, ids, caps, KV, 20, by="sum")
    t = host["totals"]
    # the size query: no out at all, and an out whose every pointer is NULL
    for want in ((), ("none",)):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, KV, 20, by="sum", cap_keys=20, units_cap=t["units_top"], max_keys=100, want=want)
        assert rc == N.GX_OK and totals == t and untouched(arrays)
    # exactly enough
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, KV, 20, by="sum", cap_keys=20, units_cap=t["units_top"], max_keys=100)
    assert rc == N.GX_OK and totals == t and np.array_equal(arrays["number"][:20], host["key_number"]) and (arrays["number"][20:].view(np.uint8) == 0xAB).all()
    assert np.array_equal(arrays["units"][:t["units_top"]], host["key_units"]) and (arrays["units"][t["units_top"]:] == 0xAB).all()
    assert np.array_equal(arrays["line_rank"][:400], host["line_rank"]) and np.array_equal(arrays["offsets"][:21], host["key_offsets"])
    # cap_keys one short, key_units_cap one short: GX_E_LIMIT, the totals filled, nothing written
    for kw in (dict(cap_keys=19, units_cap=t["units_top"]), dict(cap_keys=20, units_cap=t["units_top"] - 1)):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, KV, 20, by="sum", max_keys=100, **kw)
        assert rc == N.GX_E_LIMIT and totals == t and untouched(arrays), kw
    # key_units alone does not need cap_keys; line_rank alone needs neither
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, KV, 20, by="sum", units_cap=t["units_top"], max_keys=100, want=("units", "line_rank"))
    assert rc == N.GX_OK and np.array_equal(arrays["units"][:t["units_top"]], host["key_units"]) and np.array_equal(arrays["line_rank"][:400], host["line_rank"])
    # the overflowed table: 100 keys in 64 slots
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, KV, 20, by="sum", cap_keys=20, units_cap=1000, max_keys=8)
    assert rc == N.GX_E_LIMIT and totals["group"]["exact"] is False and totals["group"]["n_keys"] == 65 and totals["n_top"] == 0 and untouched(arrays)
    # ... and the wrapper's way out of it
    again = gorp.top_groups(data, offsets, ids, caps, KV, 20, by="sum", keys="csr", max_keys=8, line_rank=True)
    assert plain(again) == plain(host)


# ---------------------------------------------------------------------------
# device buffers, streams, determinism, whole files
# ---------------------------------------------------------------------------
@pytest.fixture
def new_stream():
    """Streams of a test's own, made with the HIP runtime and destroyed behind the test -- not taken from torch's pool, which hands its
    32 streams out in turn: the streams that the test files behind this one get, and the hardware queues they share with the default
    stream, are what they would be without this file."""
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


def on_device(gorp, data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, n_wanted, cap_keys, units_cap, **kw):
    """top_groups_device with torch buffers, every one poisoned.  Returns (rc, totals, dict of host arrays)."""
    import torch
    units = torch.full((units_cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    koff = torch.full((cap_keys + 1 + 4,), -1, dtype=torch.int32, device="cuda")
    number = torch.full((cap_keys + 4,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((cap_keys + 4,), -1, dtype=torch.int32, device="cuda")
    lines = torch.full((cap_keys + 4,), -1, dtype=torch.int64, device="cuda")
    stats = torch.full((cap_keys + 4, 8), -1, dtype=torch.int64, device="cuda")
    lrank = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc, totals = gorp.top_groups_device(data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, n_wanted, key_units_ptr=units.data_ptr(), key_units_cap=units_cap,
                                        key_offsets_ptr=koff.data_ptr(), key_number_ptr=number.data_ptr(), key_first_line_ptr=first.data_ptr(),
                                        key_lines_ptr=lines.data_ptr(), key_stats_ptr=stats.data_ptr(), line_rank_ptr=lrank.data_ptr(), cap_keys=cap_keys, **kw)
    torch.cuda.synchronize()
    k, u = (totals["n_top"], totals["units_top"]) if rc == N.GX_OK else (0, 0)
    wrote_rank = rc == N.GX_OK
    assert (units[u:] == 0x5A).all() and (koff[k + 1:] == -1).all() and (number[k:] == -1).all() and (first[k:] == -1).all() and (stats[k:] == -1).all()
    assert (lrank[n:] == 0x5A5A5A5A).all() and (wrote_rank or (lrank == 0x5A5A5A5A).all())
    return rc, totals, {"key_units": units[:u].cpu().numpy(), "key_offsets": koff[:k + 1].cpu().numpy().view(np.uint32), "key_number": number[:k].cpu().numpy().view(np.uint32),
                        "first_line": first[:k].cpu().numpy().view(np.uint32), "lines": lines[:k].cpu().numpy().view(np.uint64), "stats": stats[:k].cpu().numpy(),
                        "line_rank": lrank[:n].cpu().numpy().view(np.uint32)}


def same_arrays(dev, host):
    for k in ("key_units", "key_offsets", "key_number", "first_line", "lines", "line_rank"):
        assert np.array_equal(dev[k], host[k]), k
    fields = ("lines", "numbers", "unset", "not_numbers")
    assert np.array_equal(dev["stats"][:, :4], np.array([[s[f] for f in fields] for s in host["stats"]], np.int64).reshape(-1, 4))
    assert [int(lo) + (int(hi) << 64) for lo, hi in zip(dev["stats"][:, 6].view(np.uint64), dev["stats"][:, 7])] == [s["sum"] for s in host["stats"]]


def test_device_pointers_give_the_same_bits_as_host_arrays_twice_and_on_a_second_stream(new_stream):
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n = 3000
    names, values, ids = rng.integers(0, 150, n), rng.integers(-10 ** 6, 10 ** 12, n), rng.integers(-2, 4, n)
    values[-1], ids[-1] = INT64_MAX, 3                                           # the last capture ends at the buffer's last byte
    data, offsets, ids, caps = numbered(names, values, ids)
    parts = [(3, 0, 1), (0, 0, 1), (1, 0)]
    d_data, d_off, d_ids, d_caps = torch.from_numpy(data).cuda(), torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    batch = (d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr())
    s1, s2 = new_stream(), new_stream()
    torch.cuda.synchronize()
    for by, largest, n_wanted in (("lines", True, 10), ("sum", True, 64), ("min", False, 150), ("max", True, 1)):
        host = check(gorp, data, offsets, ids, caps, parts, n_wanted, by=by, largest=largest)
        k, units = host["totals"]["n_top"], host["totals"]["units_top"]
        rc, totals, dev = on_device(gorp, *batch, parts, n_wanted, k, units, by=by, largest=largest, max_keys=150)
        assert rc == N.GX_OK and totals == host["totals"]
        same_arrays(dev, host)
        # two calls on the same batch: the same bytes in every output
        rc, totals2, again = on_device(gorp, *batch, parts, n_wanted, k + 3, units + 5, by=by, largest=largest, max_keys=n)
        assert rc == N.GX_OK and totals2 == totals and all(dev[f].tobytes() == again[f].tobytes() for f in dev)
        # a call on a second stream right behind a device_pointers call on the first, whose emit may still be running
        number1 = torch.full((k + 1,), -1, dtype=torch.int32, device="cuda")
        lrank1 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        rc1, _ = gorp.top_groups_device(*batch, parts, n_wanted, by=by, largest=largest, key_number_ptr=number1.data_ptr(), line_rank_ptr=lrank1.data_ptr(), cap_keys=k,
                                        max_keys=150, stream=s1.cuda_stream)
        rc2, totals3, other = on_device(gorp, *batch, [(0, 0, 1)], 5, 5, 64, by="numbers", max_keys=150, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert rc1 == rc2 == N.GX_OK
        assert np.array_equal(number1[:k].cpu().numpy().view(np.uint32), host["key_number"]) and np.array_equal(lrank1.cpu().numpy().view(np.uint32), host["line_rank"])
        want = gorp.top_groups(data, offsets, ids, caps, [(0, 0, 1)], 5, by="numbers", keys="csr", line_rank=True)
        assert totals3 == want["totals"]
        same_arrays(other, want)
    # too small on the device: nothing written (on_device looks at every buffer)
    rc, totals, dev = on_device(gorp, *batch, parts, 10, 9, 1000, max_keys=150)
    assert rc == N.GX_E_LIMIT and totals["n_top"] == 10


def text_lines(n, seed, utf8):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        verb = rng.choice(["GET"] * 4 + ["PUT"] * 3 + ["POST", "DELETE", "HEAD"])
        ms = rng.choice([rng.randrange(0, 10), rng.randrange(0, 1000), rng.randrange(0, 100000), 500, 499, 7]) if rng.random() < 0.9 else "007"
        path = "/" + rng.choice(["v1/", "v2/", "café/", "Ж€/"] if utf8 else ["v1/", "v2/", "api/v1/x", ""]) + "x" * rng.randrange(0, 6)
        line = "[%d]: %s %sms %s" % (rng.randrange(1, 10 ** 9), verb, ms, path)
        r = rng.random()
        if r < 0.08:
            line = line.replace("]: ", "]; ")                       # no extraction matches
        elif r < 0.12:
            line = ""
        out.append(line)
    return out


@pytest.mark.parametrize("utf8", [False, True])
def test_text_top_groups_is_split_extract_top_groups(utf8, new_stream):
    import torch
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in text_lines(2000, 21, utf8)]
    text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 777ms /tail"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
    # the verbs by their lines and by the sum of timeTakenInMsec; the paths likewise, with a term
    for parts, by, largest, n, where in ((BY_VERB, "lines", True, 3, None), (BY_VERB, "sum", True, 10, None), (BY_PATH, "sum", False, 7, [("GetRequest", TIME, ">=", 500)]),
                                         (BY_PATH, "max", True, 5, None)):
        want = check(gorp, data, offsets, ids, caps, parts, n, by=by, largest=largest, where=where, utf8="bytes" if utf8 else None)
        got, counts, n_lines = gorp.text_top_groups(text, parts, n, by=by, largest=largest, where=where, utf8=utf8, keys="csr", line_rank=True)
        assert plain(got) == plain(want) and n_lines == len(raw) + 1 == len(got["line_rank"])
        assert np.array_equal(counts, gorp.count_outcomes(ids))
    got, counts, n_lines = gorp.text_top_groups(b"", BY_VERB, 5, utf8=utf8)
    assert n_lines == 0 and got["keys"] == [] and got["totals"]["n_top"] == 0
    # device outputs are complete when the call returns: the next whole-file call, on another stream, takes the handle's buffers
    k = want["totals"]["n_top"]
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, np.uint8).copy()).cuda()
    other = "".join("[%d]: PUT %dms /x%d\n" % (j, j, j) for j in range(50000)).encode()
    d_other = torch.from_numpy(np.frombuffer(other + b"\0" * 16, np.uint8).copy()).cuda()
    s1, s2 = new_stream(), new_stream()
    d_number = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    d_rank = torch.full((len(raw) + 1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, totals, _, nl = gorp.text_top_groups_device(d_text.data_ptr(), len(text), BY_PATH, 5, by="max", key_number_ptr=d_number.data_ptr(), line_rank_ptr=d_rank.data_ptr(),
                                                    cap_keys=k, max_keys=len(raw) + 1, stream=s1.cuda_stream, utf8=utf8)
    gorp.text_capture_stats_device(d_other.data_ptr(), len(other), [("PutRequest", TIME)], stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals == want["totals"] and nl == len(raw) + 1
    assert np.array_equal(d_number.cpu().numpy().view(np.uint32), want["key_number"]) and np.array_equal(d_rank.cpu().numpy().view(np.uint32), want["line_rank"])
