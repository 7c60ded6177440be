"""GPU tests of gx_group_quantiles / gx_text_group_quantiles: percentiles of a captured number per captured text.

Expected values come from tests/group_quantile_oracle.py -- group_oracle.group_lines for the keys, line_key and the stats, and per key
quantile_oracle.quantiles_of over that key's numbers -- and everything is compared bit for bit.  Most batches are fabricated against
handles of K identical, trivial extractions with two groups: a line is "key value", its capture row (0, |key|, |key| + 1, |line|), its id
chosen here; the end-to-end cases take ids and rows from gx_extract_batch.  The large shapes are compared with a numpy restatement:
a sort by (key number, value)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, lines_to_csr, split_lines
from group_oracle import decode_parts
from group_quantile_oracle import check_invariants, group_quantiles, plan_of, same_quantiles
from quantile_oracle import ASKS, INT64_MAX, INT64_MIN, parting_values, rank_of
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4 * 64 * int(re.search(r"GQ_TILES = (\d+)", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_group_quantile.hip")).read()).group(1))   # pairs a sort workgroup owns
P = [(50, 100), (95, 100), (99, 100)]
ENDS = [(0, 1), (1, 2), (1, 1)]
TIME = "timeTakenInMsec"
BY_VERB = [("PutRequest", "verb", TIME), ("GetRequest", "verb", TIME), ("OtherRequest", "verb", TIME)]
BY_PATH = [("PutRequest", "path", TIME), ("GetRequest", "path", TIME), ("OtherRequest", "path", TIME)]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, asks, where=None, utf8=None, **kw):
    """group_quantiles against the restatement, every field, and the invariants; returns what the call returned."""
    p = gorp.group_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = group_quantiles(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions, asks)
    got = gorp.group_quantiles(data, offsets, ids, caps, p, asks, where=terms, utf8=utf8, keys="csr", **kw)
    same_quantiles(got, want, asks, data.dtype)
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
    lines = [list(k) + [0x20] + list(v) for k, v in zip(keys, values)]
    offsets = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(offsets_dtype)
    data = np.array([u for ln in lines for u in ln], dtype=dtype)
    caps = np.array([[0, len(k), len(k) + 1, len(k) + 1 + len(v)] for k, v in zip(keys, values)], np.int32).reshape(len(lines), 4)
    return data, offsets, np.zeros(len(lines), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def numbered(key_numbers, numbers, ids=None):
    """kv_batch of key numbers (spelled k<number>) and int values"""
    return kv_batch([b"k%d" % k for k in key_numbers], [b"%d" % v for v in numbers], ids)


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def np_rows(key_of_line, values, asks):
    """The restatement for large fabricated batches where every line has a key and a number: the keys numbered by first appearance, a
    sort by (key number, value), and per (key, quantile) an index into the key's run.  Returns (n_keys, int64 [n_keys][n_q][4])."""
    key_of_line, values = np.asarray(key_of_line), np.asarray(values, np.int64)
    uniq, first, inverse = np.unique(key_of_line, return_index=True, return_inverse=True)
    number = np.empty(len(uniq), np.int64)
    number[np.argsort(first)] = np.arange(len(uniq))
    knum = number[inverse]
    order = np.lexsort((values, knum))
    sk, sv = knum[order], values[order]
    starts = np.searchsorted(sk, np.arange(len(uniq)), side="left")
    ends = np.searchsorted(sk, np.arange(len(uniq)), side="right")
    out = np.zeros((len(uniq), len(asks), 4), np.int64)
    for j in range(len(uniq)):
        run = sv[starts[j]:ends[j]]
        for q, (num, den) in enumerate(asks):
            r = rank_of(num, den, len(run))
            v = run[r - 1]
            lo = int(np.searchsorted(run, v, side="left"))
            out[j, q] = (v, r, lo, int(np.searchsorted(run, v, side="right")) - lo)
    return len(uniq), out


def rows_array(quantiles):
    return np.array([[[r["value"] or 0, r["rank"], r["below"], r["equal"]] for r in rows] for rows in quantiles], np.int64).reshape(len(quantiles), -1, 4)


def raw_call(gorp, data, offsets, ids, caps, parts, asks, max_keys=0, units_cap=0, want=("units", "offsets", "first", "lines", "stats", "line_key", "rows"), flags=0,
             poison=0xAB, quantiles=True, **kw):
    """gx_group_quantiles (quantiles=False: gx_group_lines) itself on host arrays whose every byte is `poison` before the call; returns
    (rc, totals dict, arrays dict)."""
    p = gorp.group_parts(parts)
    qarr, n_q = Gorp.quantile_asks(asks)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"units": np.full(units_cap + 8, poison, data.dtype), "offsets": np.full(max_keys + 1 + 8, poison, np.uint32).view(offsets.dtype),
              "first": np.full(max_keys + 8, poison, np.uint32), "lines": np.full(max_keys + 8, poison, np.uint64),
              "stats": np.full((max_keys + 8) * 64, poison, np.uint8), "line_key": np.full(n + 8, poison, np.uint32),
              "rows": np.full((max_keys * max(1, n_q) + 8) * 32, poison, np.uint8)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_group_out(ptr("units"), units_cap, ptr("offsets"), ptr("first"), ptr("lines"), ptr("stats") if p.has_values else None, ptr("line_key"), max_keys)
    totals = N.gx_group_totals()
    batch = (gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
             None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0)
    if quantiles:
        rc = N.lib().gx_group_quantiles(*batch, qarr, n_q, flags, C.byref(out), ptr("rows"), C.byref(totals), C.byref(o))
    else:
        rc = N.lib().gx_group_lines(*batch, flags, C.byref(out), C.byref(totals), C.byref(o))
    return rc, Gorp._group_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


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
    by_verb = check(gorp, data, offsets, id_col, rows, BY_VERB, P)
    assert len(by_verb["quantiles"]) == 6 and all(len(rows_) == 3 for rows_ in by_verb["quantiles"]) and by_verb["key_offsets"].dtype == offsets_dtype
    # p50 / p95 / p99 of timeTakenInMsec per verb is gx_capture_quantiles with an == term per verb: the loop a caller had to write
    listed = gorp.group_quantiles(data, offsets, id_col, rows, BY_VERB, P)
    by = [("PutRequest", TIME), ("GetRequest", TIME), ("OtherRequest", TIME)]
    for verb, rows_ in zip(listed["keys"], listed["quantiles"]):
        spec = [(name, "verb", "==", verb) for name in ("PutRequest", "GetRequest", "OtherRequest")]
        assert gorp.capture_quantiles(data, offsets, id_col, rows, by, P, where=spec)[0] == rows_
    by_path = check(gorp, data, offsets, id_col, rows, BY_PATH, P)
    assert by_path["totals"]["n_keys"] > 500
    # the numbers of all keys are the numbers capture_quantiles totals for the same parts: every counted line has a key here
    whole = gorp.capture_quantiles(data, offsets, id_col, rows, by, P)[1]
    assert sum(s["numbers"] for s in by_path["stats"]) == whole["numbers"] == sum(s["numbers"] for s in by_verb["stats"])


def test_terms_and_parts_that_share_one_key_space(readme):
    gorp, data, offsets, ids, caps = readme
    without = check(gorp, data, offsets, ids, caps, BY_VERB, P + ENDS)
    got = check(gorp, data, offsets, ids, caps, BY_VERB, P + ENDS, where=[("GetRequest", TIME, ">=", 500), ("OtherRequest", "verb", "!=", "POST")])
    assert got["totals"]["lines"] < without["totals"]["lines"] and len(got["quantiles"]) == 5
    # two parts, one key space: GetRequest measured, PutRequest only counted -- the paths they share have GetRequest's numbers alone
    mixed = check(gorp, data, offsets, ids, caps, [("GetRequest", "path", TIME), ("PutRequest", "path")], P)
    only = check(gorp, data, offsets, ids, caps, [("GetRequest", "path", TIME)], P)
    keys = lambda r: [bytes(r["key_units"][r["key_offsets"][j]:r["key_offsets"][j + 1]]) for j in range(len(r["lines"]))]
    mixed_rows = dict(zip(keys(mixed), mixed["quantiles"]))
    assert len(mixed_rows) > len(only["quantiles"]) and all(mixed_rows[k] == rows_ for k, rows_ in zip(keys(only), only["quantiles"]))
    # no part has a value: every row is zeros; no parts at all: no keys
    none = check(gorp, data, offsets, ids, caps, [("GetRequest", "verb")], P)
    assert none["stats"] is None and none["quantiles"] == [[{"value": None, "rank": 0, "below": 0, "equal": 0}] * 3]
    assert check(gorp, data, offsets, ids, caps, [], P)["quantiles"] == []


# ---------------------------------------------------------------------------
# one key: gx_capture_quantiles of the batch; every line its own key; run boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [B - 1, B, B + 1, 3 * B + 7])
def test_one_key_on_every_line_equals_capture_quantiles(n):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n)
    values = rng.integers(-300, 300, n) if n % 2 else rng.integers(-2 ** 62, 2 ** 62, n)
    data, offsets, ids, caps = numbered(np.zeros(n, np.int64), values)
    got = gorp.group_quantiles(data, offsets, ids, caps, [(0, 0, 1)], ASKS, keys="csr")
    whole, totals = gorp.capture_quantiles(data, offsets, ids, caps, [(0, 1)], ASKS)
    assert got["quantiles"] == [whole] and totals["numbers"] == n == got["stats"][0]["numbers"] and got["totals"]["n_keys"] == 1
    assert np.array_equal(rows_array(got["quantiles"]), np_rows(np.zeros(n), values, ASKS)[1])
    check_invariants(got, ASKS)


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097])
def test_every_line_its_own_key(n):
    """every run has length 1: one, two and three key digits are sorted"""
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n)
    values = rng.integers(-10 ** 9, 10 ** 9, n)
    data, offsets, ids, caps = numbered(rng.permutation(n), values)
    got = gorp.group_quantiles(data, offsets, ids, caps, [(0, 0, 1)], P + ENDS, keys="csr", max_keys=n, key_units_cap=8 * n)
    assert got["totals"]["n_keys"] == n and np.array_equal(got["line_key"], np.arange(n))
    want = np.zeros((n, 6, 4), np.int64)
    want[:, :, 0], want[:, :, 1], want[:, :, 3] = values[:, None], 1, 1
    assert np.array_equal(rows_array(got["quantiles"]), want)
    check_invariants(got, P + ENDS)


RUNS = {"two keys in turn": np.arange(2 * B + 3) % 2,
        "three keys in turn": np.arange(2 * B + 3) % 3,
        # a key's run starts and ends inside, on and across a workgroup's B pairs
        "long blocks": np.repeat(np.arange(8), [B - 1, 1, B, B + 1, 5, 2 * B, B - 6, 3]),
        "blocks that come back": np.repeat([0, 1, 0, 2, 1, 0], [B // 2, B, B // 2 + 1, 7, B - 8, B])}


@pytest.mark.parametrize("shape", sorted(RUNS))
def test_run_boundaries(shape):
    gorp = trivial_handle(1)
    keys = RUNS[shape]
    rng = np.random.default_rng(len(keys))
    values = rng.integers(0, 1000, len(keys))
    data, offsets, ids, caps = numbered(keys, values)
    got = gorp.group_quantiles(data, offsets, ids, caps, [(0, 0, 1)], ASKS, keys="csr")
    n_keys, want = np_rows(keys, values, ASKS)
    assert got["totals"]["n_keys"] == n_keys and np.array_equal(rows_array(got["quantiles"]), want)
    assert got["lines"].tolist() == [int((keys == k).sum()) for k in range(n_keys)]
    check_invariants(got, ASKS)


# ---------------------------------------------------------------------------
# which digits are sorted
# ---------------------------------------------------------------------------
BASE = 0x0123456789ABCDEF


def one_digit(d, count):
    return [((BASE & ~(63 << (6 * d))) | (((x * 5) % 64) << (6 * d))) % 2 ** 64 - 2 ** 63 for x in range(count)]


DIGITS = {"every value digit": [sum(((j * 7 + d) % 64) << (6 * d) for d in range(11)) % 2 ** 64 - 2 ** 63 for j in range(64)],
          "parting values": parting_values(),
          "all values equal": [1234567],
          "the top digit alone": one_digit(10, 16),
          "the bottom digit alone": one_digit(0, 64),
          "the sign alone": [INT64_MIN + 5, 5],
          "the ends of int64": [INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1, INT64_MAX - 1]}


@pytest.mark.parametrize("name", sorted(DIGITS))
def test_digits(name):
    gorp = trivial_handle(2)
    pool = DIGITS[name]
    mask = plan_of(pool, 1)[0]
    assert {"every value digit": mask == 2047, "all values equal": mask == 0, "the top digit alone": mask == 1 << 10, "the bottom digit alone": mask == 1,
            "the sign alone": mask == 1 << 10}.get(name, mask != 0)
    rng = np.random.default_rng(len(pool))
    n = 700
    values = [pool[j] for j in rng.integers(0, len(pool), n)]
    keys = rng.integers(0, 5, n)
    data, offsets, ids, caps = numbered(keys, values, rng.integers(0, 2, n))
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (1, 0, 1)], ASKS)
    assert np.array_equal(rows_array(got["quantiles"]), np_rows(keys, values, ASKS)[1])


# ---------------------------------------------------------------------------
# classes: keys without numbers, numbers without a key, a part that only counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_keys_without_numbers_numbers_without_a_key_and_a_part_that_only_counts(fmt):
    gorp = trivial_handle(3)
    rng = random.Random(9)
    keys, values, ids, unkeyed, unvalued = [], [], [], [], []
    for i in range(900):
        key = rng.choice([b"num", b"num2", b"words", b"unset", b"mixed", b"count-only"])
        value = {b"words": rng.choice([b"x", b"", b"1e3", b"99999999999999999999"]), b"mixed": rng.choice([b"7", b"x", b"-7", b"+7"])}.get(key, b"%d" % rng.randrange(-50, 50))
        keys.append(key)
        values.append(value)
        ids.append(2 if key == b"count-only" else rng.choice([0, 0, 1, -1, -2]))
        unkeyed.append(key in (b"num", b"mixed") and rng.random() < 0.2)          # a number, and a key pair that names no value
        unvalued.append(key == b"unset" or (key == b"mixed" and rng.random() < 0.2))
    data, offsets, ids, caps = kv_batch(keys, values, ids)
    caps[np.array(unkeyed), 0:2] = rng.choice([(-1, -1), (3, 2), (-1, 2)])
    caps[np.array(unvalued), 2:4] = -1
    id_col, rows = (ids, caps) if fmt == "int32" else (pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8), None)
    parts = [(0, 0, 1), (1, 0, 1), (2, 0)]
    got = check(gorp, data, offsets, id_col, rows, parts, ASKS)
    listed = gorp.group_quantiles(data, offsets, id_col, rows, parts, ASKS)
    by_key = dict(zip(listed["keys"], zip(listed["stats"], listed["quantiles"])))
    zero = {"value": None, "rank": 0, "below": 0, "equal": 0}
    for key in (b"words", b"unset", b"count-only"):
        assert by_key[key][0]["numbers"] == 0 and by_key[key][1] == [zero] * 16
    assert by_key[b"words"][0]["not_numbers"] > 50 and by_key[b"unset"][0]["unset"] > 50 and by_key[b"count-only"][0]["lines"] == 0
    assert by_key[b"mixed"][0]["numbers"] > 20 and by_key[b"mixed"][0]["not_numbers"] > 5 and by_key[b"mixed"][0]["unset"] > 5
    # lines with a number and no key join no population: the keys' numbers are capture_quantiles' numbers of the keyed lines alone
    whole = gorp.capture_quantiles(data, offsets, id_col, rows, [(0, 1), (1, 1)], [])[1]
    keyed = gorp.capture_quantiles(data, offsets, id_col, rows, [(0, 1), (1, 1)], [], where=[(0, 0, "set"), (1, 0, "set")])[1]
    assert got["totals"]["unset"] > 20 and sum(s["numbers"] for s in got["stats"]) == keyed["numbers"] < whole["numbers"]


# ---------------------------------------------------------------------------
# equivalences
# ---------------------------------------------------------------------------
def test_no_quantiles_is_group_lines_bit_for_bit_and_the_weak_hash_changes_nothing():
    gorp = trivial_handle(2)
    rng = np.random.default_rng(3)
    n = 3000
    keys, values = rng.integers(0, 150, n), rng.integers(-1000, 1000, n)
    data, offsets, ids, caps = numbered(keys, values, rng.integers(-1, 2, n))
    parts = [(0, 0, 1), (1, 0, 1)]
    strong = check(gorp, data, offsets, ids, caps, parts, ASKS)
    k, units = strong["totals"]["n_keys"], strong["totals"]["key_units"]
    rc0, totals0, lines_only = raw_call(gorp, data, offsets, ids, caps, parts, [], max_keys=k, units_cap=units, quantiles=False)
    rc1, totals1, no_q = raw_call(gorp, data, offsets, ids, caps, parts, [], max_keys=k, units_cap=units)
    assert rc0 == rc1 == N.GX_OK and totals0 == totals1 and all(np.array_equal(lines_only[a], no_q[a]) for a in lines_only)
    assert (no_q["rows"] == 0xAB).all()                                            # key_quantiles is not touched
    # sixteen quantiles, repeated and out of order; the rows behind the last key stay as they were
    rc2, totals2, full = raw_call(gorp, data, offsets, ids, caps, parts, ASKS, max_keys=k, units_cap=units)
    assert rc2 == N.GX_OK and totals2 == totals0 and all(np.array_equal(lines_only[a], full[a]) for a in lines_only if a != "rows")
    rows = full["rows"][:k * 16 * 32].view(np.int64).reshape(k, 16, 4)
    assert np.array_equal(rows, rows_array(strong["quantiles"])) and (full["rows"][k * 16 * 32:] == 0xAB).all()
    for a, b in ((2, 3), (0, 11), (1, 10)):                                        # ASKS' repeats
        assert np.array_equal(rows[:, a], rows[:, b])
    rc3, totals3, weak = raw_call(gorp, data, offsets, ids, caps, parts, ASKS, max_keys=k, units_cap=units, flags=N.GX_GROUP_WEAK_HASH)
    assert rc3 == N.GX_OK and totals3 == totals2 and all(np.array_equal(full[a], weak[a]) for a in full)
    assert plain(check(gorp, data, offsets, ids, caps, parts, ASKS, weak_hash=True)) == plain(strong)


# ---------------------------------------------------------------------------
# capacities
# ---------------------------------------------------------------------------
def test_capacities_the_size_query_and_the_full_table():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(23)
    n = 900
    keys, values = np.concatenate([rng.integers(0, 40, n - 40), np.arange(40)]), rng.integers(0, 100, n)
    data, offsets, ids, caps = numbered(keys, values)
    parts = [(0, 0, 1)]
    want = check(gorp, data, offsets, ids, caps, parts, P)
    k, units = want["totals"]["n_keys"], want["totals"]["key_units"]
    assert k == 40
    # the size query: no output at all, key_quantiles == NULL with n_quantiles > 0; no gx_group_out either
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=1, want=())
    assert rc == N.GX_OK and totals == want["totals"] and untouched(arrays)
    p, (qarr, n_q), t = gorp.group_parts(parts), Gorp.quantile_asks(P), N.gx_group_totals()
    batch = (gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, None, 0, qarr, n_q, 0)
    assert N.lib().gx_group_quantiles(*batch, None, None, C.byref(t), None) == N.GX_OK and Gorp._group_totals(t) == want["totals"]
    # out == NULL gives key_quantiles the capacity 0
    rows = np.full(k * 3 * 32, 0xAB, np.uint8)
    assert N.lib().gx_group_quantiles(*batch, None, rows.ctypes.data, C.byref(t), None) == N.GX_E_LIMIT
    assert Gorp._group_totals(t) == want["totals"] and (rows == 0xAB).all()
    # the keys alone, and key_quantiles alone
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=k, units_cap=units, want=("units", "offsets", "first", "lines", "stats", "line_key"))
    assert rc == N.GX_OK and (arrays["rows"] == 0xAB).all() and np.array_equal(arrays["first"][:k], want["first_line"])
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=k, want=("rows",))
    assert rc == N.GX_OK and np.array_equal(arrays["rows"][:k * 3 * 32].view(np.int64).reshape(k, 3, 4), rows_array(want["quantiles"]))
    assert (arrays["rows"][k * 3 * 32:] == 0xAB).all() and (arrays["first"].view(np.uint8) == 0xAB).all()
    # max_keys one short with key_quantiles given: GX_E_LIMIT, the poisoned outputs untouched, the totals filled
    for wanted in (("rows",), ("units", "offsets", "first", "lines", "stats", "line_key", "rows")):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=k - 1, units_cap=units, want=wanted)
        assert rc == N.GX_E_LIMIT and totals == want["totals"] and untouched(arrays), wanted
    # line_key alone has no per-key capacity, with quantiles asked for and not taken
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=k - 1, want=("line_key",))
    assert rc == N.GX_OK and np.array_equal(arrays["line_key"][:n], want["line_key"])
    # 200 keys in a table of 64 slots: not exact, nothing written; the wrapper retries with the number of lines
    keys = np.concatenate([rng.permutation(200), rng.permutation(200)])
    values = rng.integers(0, 100, 400)
    data, offsets, ids, caps = numbered(keys, values)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, P, max_keys=1, units_cap=10 ** 6)
    assert rc == N.GX_E_LIMIT and not totals["exact"] and totals["n_keys"] == 65 and totals["lines"] == 400 and untouched(arrays)
    got = check(gorp, data, offsets, ids, caps, parts, P, max_keys=1, key_units_cap=1)
    assert got["totals"]["n_keys"] == 200 and np.array_equal(rows_array(got["quantiles"]), np_rows(keys, values, P)[1])


# ---------------------------------------------------------------------------
# units
# ---------------------------------------------------------------------------
def test_utf16_units_and_utf8_bytes_with_a_key_that_is_not_ascii():
    gorp = trivial_handle(2)
    rng = random.Random(16)
    pool = [[0x31], [0xFF11], [0x31, 0xFF11], [0x416, 0x16], [0x16, 0x416], []]
    keys = [rng.choice(pool) for _ in range(400)]
    values = [rng.choice([[0x35], [0x2D, 0x37], [0xFF15], [0x31, 0x32, 0x33], []]) for _ in range(400)]      # U+FF15 is no number
    data, offsets, ids, caps = kv_batch(keys, values, [rng.choice([0, 1, -1]) for _ in range(400)], dtype=np.uint16)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (1, 0, 1)], P + ENDS)
    assert got["totals"]["n_keys"] == 6 and got["key_units"].dtype == np.uint16 and sum(s["not_numbers"] for s in got["stats"]) > 50
    assert plain(check(gorp, data, offsets, pack(ids, caps, np.uint8), None, [(0, 0, 1), (1, 0, 1)], P + ENDS)) == plain(got)
    # UTF-8 bytes of the README definition's lines
    gorp = Gorp.construct(W.readme3_definition())
    lines = []
    for j in range(1500):
        verb = rng.choice(["GET", "GET", "PUT", "POST"])
        lines.append("[%d]: %s %dms /%s%s" % (rng.randrange(1, 10 ** 9), verb, rng.choice([7, 499, 500, rng.randrange(0, 100000)]), rng.choice(["v1/", "café/", "Ж€/"]),
                                              "x" * rng.randrange(0, 4)))
    data, offsets = lines_to_csr([ln.encode("utf-8") for ln in lines])
    ids, caps = gorp.extract_batch(data, offsets, utf8="bytes")
    got = check(gorp, data, offsets, ids, caps, BY_PATH, P, utf8="bytes")
    listed = gorp.group_quantiles(data, offsets, ids, caps, BY_PATH, P, utf8="bytes")
    assert got["totals"]["n_keys"] == 12 and "/café/" in listed["keys"] and listed["quantiles"] == got["quantiles"]
    check(gorp, data, offsets, ids, caps, BY_PATH, P, where=[("GetRequest", "path", "contains", "café")], utf8="bytes")


# ---------------------------------------------------------------------------
# device buffers: alignment, stream order, determinism, whole files
# ---------------------------------------------------------------------------
@pytest.fixture
def new_stream():
    """Streams of a test's own, made with the HIP runtime and destroyed behind the test -- not taken from torch's pool, which hands its
    32 streams out in turn: the streams that the test files behind this one get, and the hardware queues they share with the default
    stream, are what they would be without this file (some of their stream-order tests depend on that)."""
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


def on_device(gorp, data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, asks, max_keys, units_cap, **kw):
    """group_quantiles_device with torch buffers, every one poisoned.  Returns (rc, totals, dict of host arrays)."""
    import torch
    n_q = len(asks)
    units = torch.full((units_cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    koff = torch.full((max_keys + 1 + 4,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((max_keys + 4,), -1, dtype=torch.int32, device="cuda")
    lines = torch.full((max_keys + 4,), -1, dtype=torch.int64, device="cuda")
    stats = torch.full((max_keys + 4, 8), -1, dtype=torch.int64, device="cuda")
    lkey = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rows = torch.full((max_keys * n_q + 4, 4), -1, dtype=torch.int64, device="cuda")
    rc, totals = gorp.group_quantiles_device(data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, asks, key_units_ptr=units.data_ptr(), key_units_cap=units_cap,
                                             key_offsets_ptr=koff.data_ptr(), key_first_line_ptr=first.data_ptr(), key_lines_ptr=lines.data_ptr(),
                                             key_stats_ptr=stats.data_ptr(), line_key_ptr=lkey.data_ptr(), key_quantiles_ptr=rows.data_ptr(), max_keys=max_keys, **kw)
    torch.cuda.synchronize()
    k, u = (totals["n_keys"], totals["key_units"]) if rc == N.GX_OK else (0, 0)
    assert (units[u:] == 0x5A).all() and (koff[k + 1:] == -1).all() and (first[k:] == -1).all() and (stats[k:] == -1).all() and (lkey[n:] == 0x5A5A5A5A).all()
    assert (rows[k * n_q:] == -1).all()                                            # nothing behind the last key's rows
    return rc, totals, {"key_units": units[:u].cpu().numpy(), "key_offsets": koff[:k + 1].cpu().numpy().view(np.uint32), "first_line": first[:k].cpu().numpy().view(np.uint32),
                        "lines": lines[:k].cpu().numpy().view(np.uint64), "stats": stats[:k].cpu().numpy(), "line_key": lkey[:n].cpu().numpy().view(np.uint32),
                        "rows": rows[:k * n_q].cpu().numpy().reshape(k, n_q, 4)}


def same_arrays(dev, host):
    for k in ("key_units", "key_offsets", "first_line", "lines", "line_key"):
        assert np.array_equal(dev[k], host[k]), k
    assert np.array_equal(dev["stats"][:, 1], [s["numbers"] for s in host["stats"]])
    assert np.array_equal(dev["rows"], rows_array(host["quantiles"]))


def test_device_buffers_at_every_misalignment():
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n = 3000
    keys, values, ids = rng.integers(0, 150, n), rng.integers(-10 ** 6, 10 ** 12, n), rng.integers(-2, 4, n)
    values[-1], ids[-1] = INT64_MAX, 3                                           # the last capture ends at the buffer's last byte
    data, offsets, ids, caps = numbered(keys, values, ids)
    rows8 = pack(ids, caps, np.uint8)
    parts = [(3, 0, 1), (0, 0, 1), (1, 0)]
    host = check(gorp, data, offsets, ids, caps, parts, P + ENDS)
    k, units = host["totals"]["n_keys"], host["totals"]["key_units"]
    d_off, d_ids, d_caps = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    for mis in (0, 1, 2, 3, 7, 8, 13, 15):
        src = torch.empty(mis + len(data), dtype=torch.uint8, device="cuda")     # sized exactly: the batch ends where the tensor ends
        src[mis:] = torch.from_numpy(data).cuda()
        rc, totals, dev = on_device(gorp, src.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), parts, P + ENDS, k, units)
        assert rc == N.GX_OK and totals == host["totals"]
        same_arrays(dev, host)
        d_rows = torch.empty(mis + rows8.size, dtype=torch.uint8, device="cuda")
        d_rows[mis:] = torch.from_numpy(rows8.reshape(-1)).cuda()
        rc, totals, dev = on_device(gorp, src.data_ptr() + mis, d_off.data_ptr(), n, d_rows.data_ptr() + mis, None, parts, P + ENDS, k + mis, units + mis, compact=2)
        assert rc == N.GX_OK
        same_arrays(dev, host)
    # too small on the device: nothing written (on_device looks at every buffer)
    rc, totals, dev = on_device(gorp, src.data_ptr() + 15, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), parts, P + ENDS, k - 1, units)
    assert rc == N.GX_E_LIMIT and totals == host["totals"]


def test_the_call_follows_a_no_sync_batch_on_its_stream_and_two_runs_are_the_same_bits(new_stream):
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 60000, 200
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    rows = torch.full((n, 1 + 2 * gorp.max_groups), 0x55, dtype=torch.uint8, device="cuda")   # ids nobody wrote: outcome 2K + 1
    stream = new_stream()
    torch.cuda.synchronize()
    where = [("GetRequest", TIME, ">=", 500)]
    batch = (data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None)
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True, compact=2,
                                  line_bytes_hint=L)
        rc, totals, got = on_device(gorp, *batch, BY_VERB, P, 6, 40, where=where, compact=2, stream=stream.cuda_stream)
        rc2, totals2, again = on_device(gorp, *batch, BY_VERB, P, 6, 40, where=where, compact=2, stream=stream.cuda_stream)
    stream.synchronize()
    assert rc == rc2 == N.GX_OK and totals == totals2 and totals["n_keys"] == 6
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k                          # two runs: the same bits
    # against the host staging of the same batch, through the loop of capture_quantiles calls
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    host = gorp.group_quantiles(h_data, h_off, h_rows, None, BY_VERB, P, where=where)
    same_arrays(got, host)
    by = [("PutRequest", TIME), ("GetRequest", TIME), ("OtherRequest", TIME)]
    for verb, rows_ in zip(host["keys"], host["quantiles"]):
        spec = where + [(name, "verb", "==", verb) for name in ("PutRequest", "GetRequest", "OtherRequest")]
        assert gorp.capture_quantiles(h_data, h_off, h_rows, None, by, P, where=spec)[0] == rows_
    # the path as key: tens of thousands of keys, claimed by whichever lane came first, delivered the same
    rc, totals, a = on_device(gorp, *batch, BY_PATH, P, n, n * L, compact=2)
    assert rc == N.GX_OK and totals["n_keys"] > n // 2
    rc, totals2, b = on_device(gorp, *batch, BY_PATH, P, n, n * L, compact=2)
    assert totals2 == totals and all(a[k].tobytes() == b[k].tobytes() for k in a)
    some = a["stats"][:, 1] > 0
    assert some.sum() > n // 2 and (a["rows"][:, :, 1] <= a["stats"][:, 1:2]).all() and (a["rows"][~some] == 0).all()
    assert (a["rows"][:, 0, 0] <= a["rows"][:, 1, 0]).all() and (a["rows"][:, 1, 0] <= a["rows"][:, 2, 0]).all() and (a["rows"][some, 2, 0] <= a["stats"][some, 5]).all()


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
def test_text_group_quantiles_is_split_extract_group_quantiles(utf8, new_stream):
    import torch
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in text_lines(3000, 21, utf8)]
    text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 777ms /tail"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
    wheres = [None, [("GetRequest", TIME, ">=", 500)]]
    for parts in (BY_VERB, BY_PATH):
        for where in wheres:
            want = check(gorp, data, offsets, ids, caps, parts, P + ENDS, where=where, utf8="bytes" if utf8 else None)
            got, counts, n_lines = gorp.text_group_quantiles(text, parts, P + ENDS, where=where, utf8=utf8, keys="csr")
            assert plain(got) == plain(want) and n_lines == len(raw) + 1 == len(got["line_key"])
            assert np.array_equal(counts, gorp.count_outcomes(ids))
    got, counts, n_lines = gorp.text_group_quantiles(b"", BY_VERB, P, utf8=utf8)
    assert n_lines == 0 and got["keys"] == [] and got["quantiles"] == []
    # device outputs are complete when the call returns: the next whole-file call, on another stream, takes the handle's buffers
    k = want["totals"]["n_keys"]
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, np.uint8).copy()).cuda()
    other = "".join("[%d]: PUT %dms /x%d\n" % (j, j, j) for j in range(50000)).encode()
    d_other = torch.from_numpy(np.frombuffer(other + b"\0" * 16, np.uint8).copy()).cuda()
    s1, s2 = new_stream(), new_stream()
    d_rows = torch.full((k * 6, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, totals, _, nl = gorp.text_group_quantiles_device(d_text.data_ptr(), len(text), BY_PATH, P + ENDS, where=wheres[1], key_quantiles_ptr=d_rows.data_ptr(), max_keys=k,
                                                         stream=s1.cuda_stream, utf8=utf8)
    now = d_rows.cpu().numpy().copy()                                              # (no wait on s1)
    gorp.text_capture_stats_device(d_other.data_ptr(), len(other), [("PutRequest", TIME)], stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals == want["totals"] and nl == len(raw) + 1
    assert np.array_equal(now.reshape(k, 6, 4), rows_array(want["quantiles"])) and np.array_equal(d_rows.cpu().numpy(), now)


# ---------------------------------------------------------------------------
# 200 k lines, about 3 000 keys of skewed sizes, against a numpy sort by (key, value)
# ---------------------------------------------------------------------------
def test_200k_lines_of_skewed_keys_against_a_numpy_sort():
    import torch
    gorp = trivial_handle(1)
    n, w = 200000, 12
    rng = np.random.default_rng(5)
    # one key holds half the lines, 400 hold about 120 each, and 2 600 share 3 000 lines: many of those hold one
    keys = np.where(rng.random(n) < 0.5, 0, np.where(rng.random(n) < 0.97, rng.integers(1, 401, n), rng.integers(401, 3001, n)))
    values = np.where(rng.random(n) < 0.9, rng.integers(0, 2000, n), rng.integers(0, 10 ** 6, n))
    # a line is five digits of the key, a blank, six digits of the value
    spell = lambda x, d: ((x[:, None] // 10 ** np.arange(d - 1, -1, -1)[None, :]) % 10 + 48).astype(np.uint8)
    table = np.concatenate([spell(keys, 5), np.full((n, 1), 0x20, np.uint8), spell(values, 6)], axis=1)
    assert table.shape == (n, w)
    data = torch.from_numpy(np.ascontiguousarray(table).reshape(-1)).cuda()
    d_off = (torch.arange(n + 1, device="cuda") * w).to(torch.int32)
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    caps = torch.tensor([0, 5, 6, 12], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
    n_keys, want = np_rows(keys, values, P + ENDS)
    sizes = np.bincount(keys)
    assert 1800 < n_keys <= 3001 and sizes[0] > 0.45 * n and (sizes == 1).sum() > 300
    rc, totals, got = on_device(gorp, data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), [(0, 0, 1)], P + ENDS, n_keys, 5 * n_keys)
    assert rc == N.GX_OK and totals["n_keys"] == n_keys and totals["keyed"] == n
    assert np.array_equal(got["rows"], want)
    assert np.array_equal(got["stats"][:, 1], got["lines"].astype(np.int64)) and got["stats"][:, 1].sum() == n
    assert np.array_equal(got["rows"][:, 3, 0], got["stats"][:, 4]) and np.array_equal(got["rows"][:, 5, 0], got["stats"][:, 5])     # num == 0: min; num == den: max
    assert (got["rows"][:, :, 2] < got["rows"][:, :, 1]).all() and (got["rows"][:, :, 1] <= got["rows"][:, :, 2] + got["rows"][:, :, 3]).all()
    assert (got["rows"][:, :, 2] + got["rows"][:, :, 3] <= got["stats"][:, 1:2]).all()
