"""GPU tests of gx_group_lines / gx_text_group_lines: the lines of a finished batch grouped by the text they captured.

Expected values come from tests/group_oracle.py -- a Python dict filled line by line, the value sliced out of the line with the capture
offsets, where_oracle.parse_long and Python's integers for the per-key sums -- and everything is compared exactly.  Most batches are
fabricated against handles of K identical, trivial extractions: a line is its value, its capture row (0, length), its id chosen here;
the end-to-end cases take ids and rows from gx_extract_batch.  The large shapes have closed forms (one key; every line its own key)
and are compared as arrays."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from group_oracle import NONE, decode_parts, group_lines, group_values, same
from stats_oracle import SUM_SEQUENCES
from where_oracle import INT64_MAX, INT64_MIN, INT_TABLE, decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUT, GET, OTHER = 0, 1, 2  # workloads.readme3_definition: the extractions' indices; groups timestamp, verb, timeTakenInMsec, path
K3 = 3
GRID_LINES = 2048 * 256    # gx_group.hip: lines of one trip of the grid stride
LDS_KEYS = int(re.search(r"GROUP_LDS_KEYS = (\d+)", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_group.hpp")).read()).group(1))
VERB_PARTS = [("PutRequest", "verb", "timeTakenInMsec"), ("GetRequest", "verb", "timeTakenInMsec"), ("OtherRequest", "verb", "timeTakenInMsec")]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, where=None, utf8=None, **kw):
    """group_lines against the restatement, every field; returns what the call returned."""
    p = gorp.group_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = group_lines(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions)
    got = gorp.group_lines(data, offsets, ids, caps, p, where=terms, utf8=utf8, keys="csr", **kw)
    same(got, want, data.dtype)
    return got


def plain(res):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}


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
    return (ids, caps) if fmt == "int32" else (pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8), None)


def raw_call(gorp, data, offsets, ids, caps, parts, max_keys=0, units_cap=0, want=("units", "offsets", "first", "lines", "stats", "line_key"), flags=0,
             poison=0xAB, **kw):
    """gx_group_lines itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.group_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"units": np.full(units_cap + 8, poison, data.dtype), "offsets": np.full(max_keys + 1 + 8, poison, np.uint32).view(offsets.dtype),
              "first": np.full(max_keys + 8, poison, np.uint32), "lines": np.full(max_keys + 8, poison, np.uint64),
              "stats": np.full((max_keys + 8) * 64, poison, np.uint8), "line_key": np.full(n + 8, poison, np.uint32)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_group_out(ptr("units"), units_cap, ptr("offsets"), ptr("first"), ptr("lines"), ptr("stats") if p.has_values else None, ptr("line_key"), max_keys)
    totals = N.gx_group_totals()
    rc = N.lib().gx_group_lines(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
                                None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, flags, C.byref(out), C.byref(totals), C.byref(o))
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
    assert (ids == GET).sum() > 500 and (ids == PUT).sum() > 500 and (ids == OTHER).sum() > 50 and (ids == -1).sum() > 10
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
        assert np.array_equal(id_col, pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8))
    got = check(gorp, data, offsets, id_col, rows, VERB_PARTS)
    assert got["key_offsets"].dtype == offsets_dtype
    listed = gorp.group_lines(data, offsets, id_col, rows, VERB_PARTS)
    assert sorted(listed["keys"]) == sorted(v.encode() for v in W.README3_VERBS) and len(listed["keys"]) == 6
    # in order of appearance: the caller's LinkedHashMap, in Python
    by_verb = {}
    for i in np.flatnonzero(ids >= 0):
        verb = bytes(data[int(offsets[i]) + caps[i, 2]:int(offsets[i]) + caps[i, 3]])
        by_verb[verb] = by_verb.get(verb, 0) + 1
    assert listed["keys"] == list(by_verb) and listed["lines"].tolist() == list(by_verb.values())
    assert got["totals"]["lines"] == got["totals"]["keyed"] == (ids >= 0).sum() and got["totals"]["unset"] == 0
    assert ((got["line_key"] == NONE) == (ids < 0)).all()
    # key_stats summed over the keys is gx_capture_stats of the same lines
    whole = gorp.capture_stats(data, offsets, id_col, rows, [("PutRequest", "timeTakenInMsec"), ("GetRequest", "timeTakenInMsec"), ("OtherRequest", "timeTakenInMsec")])
    for field in ("lines", "numbers", "unset", "not_numbers", "sum"):
        assert sum(s[field] for s in got["stats"]) == sum(s[field] for s in whole)
    assert min(s["min"] for s in got["stats"]) == min(s["min"] for s in whole) and max(s["max"] for s in got["stats"]) == max(s["max"] for s in whole)
    # key_lines is gx_select_lines_where(==) per key
    for verb, count in zip(listed["keys"], listed["lines"]):
        spec = [(name, "verb", "==", verb) for name in ("PutRequest", "GetRequest", "OtherRequest")]
        assert len(gorp.select_lines_where(data, offsets, id_col, rows, spec)[0]) == count


def test_terms_restrict_the_lines(readme):
    gorp, data, offsets, ids, caps = readme
    without = check(gorp, data, offsets, ids, caps, VERB_PARTS)
    specs = [[("GetRequest", "timeTakenInMsec", ">=", 500)],
             [("GetRequest", "timeTakenInMsec", "<", 500), ("OtherRequest", "verb", "!=", "POST")],
             [("PutRequest", "path", "contains", "a"), ("OtherRequest", "verb", "unset")]]
    for fmt in ("int32", "u8"):
        id_col, rows = (ids, caps) if fmt == "int32" else (gorp.extract_batch(data, offsets, compact=2)[0], None)
        for spec in specs:
            got = check(gorp, data, offsets, id_col, rows, VERB_PARTS, where=spec)
            assert got["totals"]["lines"] < without["totals"]["lines"]
    assert len(check(gorp, data, offsets, ids, caps, VERB_PARTS, where=specs[1])["lines"]) == 5          # POST is gone
    assert len(check(gorp, data, offsets, ids, caps, VERB_PARTS, where=specs[2])["lines"]) == 2          # ... and every other verb
    # a part for one extraction only; the path as key (long, nearly all distinct); no parts at all
    assert check(gorp, data, offsets, ids, caps, [("GetRequest", "verb")])["lines"].tolist() == [(ids == GET).sum()]
    paths = check(gorp, data, offsets, ids, caps, [("GetRequest", "path", "timeTakenInMsec"), ("OtherRequest", "path")])
    assert paths["totals"]["n_keys"] > 500 and paths["totals"]["key_units"] > 50 * paths["totals"]["n_keys"]
    none = check(gorp, data, offsets, ids, caps, [])
    assert none["totals"] == {"n_keys": 0, "key_units": 0, "lines": 0, "keyed": 0, "unset": 0, "exact": True} and (none["line_key"] == NONE).all()
    assert none["key_offsets"].tolist() == [0]


# ---------------------------------------------------------------------------
# the empty value, unset pairs, pairs outside their line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_the_empty_value_is_a_key_and_pairs_that_name_no_value_are_not(fmt):
    gorp = trivial_handle(2, groups=2)
    pairs = [(-1, -1), (0, 0), (-1, 3), (5, 5), (3, 2), (0, 5), (0, 6), (2, 2), (5, 6), (6, 6), (2, 4), (0, 0), (-1, -1)]   # the line is b"12345"
    lines, caps, ids = [], [], []
    for rep in range(3):
        for k in (0, 1):
            for b, e in pairs:
                lines.append(b"12345")
                caps.append([b, e, 1, 3] if rep != 1 else [b, e, -1, -1])
                ids.append(k)
    lines.append(b"7")                                          # (the last line: "beyond the line" above stays inside the buffer)
    caps.append([0, 1, 0, 1])
    ids.append(0)
    data, offsets = csr(lines)
    ids, caps = np.array(ids, np.int32), np.array(caps, np.int32)
    id_col, rows = in_format(ids, caps, fmt)
    got = check(gorp, data, offsets, id_col, rows, [(0, 0, 1), (1, 0)])
    bad = np.array([not (0 <= b <= e <= 5) for b, e in pairs] * 6 + [False])
    assert bad.sum() == 7 * 6 and got["totals"]["unset"] == bad.sum() and got["totals"]["lines"] == len(lines) == got["totals"]["keyed"] + got["totals"]["unset"]
    assert ((got["line_key"] == NONE) == bad).all()
    keys = [bytes(got["key_units"][got["key_offsets"][j]:got["key_offsets"][j + 1]]) for j in range(len(got["lines"]))]
    assert keys == [b"", b"12345", b"34", b"7"] and got["lines"].tolist() == [6 * 4, 6, 6, 1]
    assert got["stats"][0]["unset"] > 0 and got["stats"][0]["numbers"] > 0 and got["stats"][3]["sum"] == 7
    count_only = check(gorp, data, offsets, id_col, rows, [(1, 0)])
    assert count_only["stats"] is None and count_only["lines"].tolist() == [3 * 4, 3, 3]


# ---------------------------------------------------------------------------
# one key on every line; every line its own key; two keys in turn
# ---------------------------------------------------------------------------
SIZES = [64, 65, 256, 257, GRID_LINES + 1]


def fixed_width(values_u8, ids):
    """n lines of the same width from a uint8 [n][w] array"""
    n, w = values_u8.shape
    offsets = (np.arange(n + 1, dtype=np.uint64) * w).astype(np.uint32)
    caps = np.tile(np.array([0, w, 0, w], np.int32), (n, 1))
    return np.ascontiguousarray(values_u8).reshape(-1), offsets, np.asarray(ids, np.int32), caps


@pytest.mark.parametrize("n", SIZES)
def test_one_key_on_every_line(n):
    gorp = trivial_handle(2, groups=2)
    data, offsets, ids, caps = fixed_width(np.tile(np.frombuffer(b"0042", np.uint8), (n, 1)), np.arange(n) % 2)
    if n <= 257:
        got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (1, 1, 0)])
    else:
        got = gorp.group_lines(data, offsets, ids, caps, [(0, 0, 1), (1, 1, 0)], keys="csr")
    assert got["totals"] == {"n_keys": 1, "key_units": 4, "lines": n, "keyed": n, "unset": 0, "exact": True}
    assert got["key_units"].tobytes() == b"0042" and got["key_offsets"].tolist() == [0, 4] and got["first_line"].tolist() == [0] and got["lines"].tolist() == [n]
    assert (got["line_key"] == 0).all() and len(got["line_key"]) == n
    assert got["stats"] == [{"lines": n, "numbers": n, "unset": 0, "not_numbers": 0, "min": 42, "max": 42, "sum": 42 * n}]


@pytest.mark.parametrize("n", SIZES)
def test_every_line_its_own_key(n):
    gorp = trivial_handle(1, groups=2)
    # seven digits of the line number, most significant first: neighbours differ in the LAST unit only
    digits = (np.arange(n)[:, None] // 10 ** np.arange(6, -1, -1)[None, :] % 10 + 48).astype(np.uint8)
    data, offsets, ids, caps = fixed_width(digits, np.zeros(n))
    if n <= 257:
        got = check(gorp, data, offsets, ids, caps, [(0, 0, 1)])
    else:
        got = gorp.group_lines(data, offsets, ids, caps, [(0, 0, 1)], keys="csr", max_keys=n, key_units_cap=7 * n)
    assert got["totals"] == {"n_keys": n, "key_units": 7 * n, "lines": n, "keyed": n, "unset": 0, "exact": True}
    assert np.array_equal(got["key_units"], data) and np.array_equal(got["key_offsets"], offsets)
    assert np.array_equal(got["first_line"], np.arange(n)) and (got["lines"] == 1).all() and np.array_equal(got["line_key"], np.arange(n))
    assert [s["sum"] for s in got["stats"][-3:]] == [n - 3, n - 2, n - 1] and all(s["numbers"] == 1 and s["min"] == s["max"] == s["sum"] for s in got["stats"][:300])


def test_values_of_equal_units_and_different_lengths_are_different_keys():
    gorp = trivial_handle(1)
    values = [b"a" * k for k in range(0, 130)] + [b"a" * k for k in range(129, -1, -1)] + [b"a" * 64 + b"b", b"a" * 63 + b"b", b"a" * 64 + b"b"]
    got = check(gorp, *values_batch(values, np.zeros(len(values))), [(0, 0)])
    assert got["totals"]["n_keys"] == 132 and got["lines"].tolist() == [2] * 131 + [1]
    assert check(gorp, *values_batch(values, np.zeros(len(values))), [(0, 0)], weak_hash=True)["totals"]["n_keys"] == 132


@pytest.mark.parametrize("n", [64, 257, 70001])
def test_two_keys_in_turn(n):
    gorp = trivial_handle(3)
    values = np.where((np.arange(n) % 2)[:, None] == 0, np.frombuffer(b"-17", np.uint8)[None, :], np.frombuffer(b"+99", np.uint8)[None, :]).astype(np.uint8)
    data, offsets, ids, caps = fixed_width(values, np.arange(n) % 3)
    caps = caps[:, :2].copy()
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 0), (2, 0, 0), (1, 0)])
    assert got["lines"].tolist() == [(n + 1) // 2, n // 2] and got["first_line"].tolist() == [0, 1]
    assert got["stats"][0]["min"] == got["stats"][0]["max"] == -17 and got["stats"][1]["sum"] == 99 * got["stats"][1]["numbers"]


# ---------------------------------------------------------------------------
# chains: the weak hash
# ---------------------------------------------------------------------------
def test_weak_hash_walks_whole_chains_and_changes_nothing():
    gorp = trivial_handle(2)
    rng = np.random.default_rng(17)
    pool = set()
    while len(pool) < 300:
        pool.add(bytes(rng.integers(0x30, 0x3A, int(rng.integers(1, 41)), dtype=np.uint8)))
    pool = sorted(pool)
    values = [pool[j] for j in rng.integers(0, 300, 2500)] + pool
    data, offsets, ids, caps = values_batch(values, rng.integers(-1, 2, len(values)))
    ids[-300:] = 0                                              # (every value of the pool is some counted line's key)
    strong = check(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0, 0)])
    weak = check(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0, 0)], weak_hash=True)
    assert plain(weak) == plain(strong) and strong["totals"]["n_keys"] == 300
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0, 0)], max_keys=300, units_cap=strong["totals"]["key_units"])
    rc2, totals2, arrays2 = raw_call(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0, 0)], max_keys=300, units_cap=strong["totals"]["key_units"],
                                     flags=N.GX_GROUP_WEAK_HASH)
    assert rc == rc2 == N.GX_OK and totals == totals2 and all(np.array_equal(arrays[k], arrays2[k]) for k in arrays)       # bit for bit, the poison behind included


# ---------------------------------------------------------------------------
# capacities
# ---------------------------------------------------------------------------
def test_capacities_the_size_query_and_the_full_table():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(23)
    pool = [b"key%03d" % j + b"x" * (j % 5) for j in range(40)]
    values = [pool[j] for j in rng.integers(0, 40, 900)] + pool
    data, offsets, ids, caps = values_batch(values, np.zeros(len(values)))
    parts = [(0, 0, 0)]
    want = check(gorp, data, offsets, ids, caps, parts)
    k, units = want["totals"]["n_keys"], want["totals"]["key_units"]
    assert k == 40
    # exactly enough
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=k, units_cap=units)
    assert rc == N.GX_OK and totals == want["totals"]
    assert np.array_equal(arrays["units"][:units], want["key_units"]) and (arrays["units"][units:].view(np.uint8) == 0xAB).all()
    assert np.array_equal(arrays["offsets"][:k + 1], want["key_offsets"]) and (arrays["offsets"][k + 1:].view(np.uint8) == 0xAB).all()
    assert np.array_equal(arrays["first"][:k], want["first_line"]) and (arrays["first"][k:].view(np.uint8) == 0xAB).all()
    assert np.array_equal(arrays["lines"][:k], want["lines"]) and (arrays["lines"][k:].view(np.uint8) == 0xAB).all()
    assert (arrays["stats"][k * 64:] == 0xAB).all() and np.array_equal(arrays["line_key"][:len(values)], want["line_key"])
    assert (arrays["line_key"][len(values):].view(np.uint8) == 0xAB).all()
    # one key short, one unit short: GX_E_LIMIT, exact totals, nothing written
    for mk, cap in ((k - 1, units), (k, units - 1), (0, 0)):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=mk, units_cap=cap)
        assert rc == N.GX_E_LIMIT and totals == want["totals"] and untouched(arrays), (mk, cap)
    # line_key alone has no per-key capacity; key_units alone needs no max_keys beyond the table's size
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=k - 1, want=("line_key",))
    assert rc == N.GX_OK and np.array_equal(arrays["line_key"][:len(values)], want["line_key"])
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=k - 1, units_cap=units, want=("units",))
    assert rc == N.GX_OK and np.array_equal(arrays["units"][:units], want["key_units"]) and (arrays["first"].view(np.uint8) == 0xAB).all()
    # the size query: every output NULL (or no gx_group_out at all), max_keys the table's size
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=1, want=())
    assert rc == N.GX_OK and totals == want["totals"] and untouched(arrays)
    t = N.gx_group_totals()
    p = gorp.group_parts(parts)
    assert N.lib().gx_group_lines(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, len(values), ids.ctypes.data, caps.ctypes.data, p.array, p.n, None, 0, 0, None,
                                  C.byref(t), None) == N.GX_OK and Gorp._group_totals(t) == want["totals"]
    # 200 distinct keys in a table of 64 slots: not exact, one more than the slots; max_keys = the lines always suffices; the wrapper retries
    pool = [b"%d" % (j * j) for j in range(200)]
    values = [pool[j] for j in rng.permutation(200)] * 2
    data, offsets, ids, caps = values_batch(values, np.zeros(len(values)))
    for want_out in ((), ("line_key",), ("units", "offsets", "first", "lines", "stats", "line_key")):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=1, units_cap=10 ** 6, want=want_out)
        assert rc == N.GX_E_LIMIT and not totals["exact"] and totals["n_keys"] == 65 and totals["lines"] == 400 and untouched(arrays)
    assert "slots" in N.last_error()
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=32, want=())
    assert rc == N.GX_E_LIMIT and totals["n_keys"] == 65
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=33, want=())                   # 128 slots for 200 keys
    assert rc == N.GX_E_LIMIT and totals["n_keys"] == 129
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=100, want=())                  # 256 slots: the query passes
    assert rc == N.GX_OK and totals["exact"] and totals["n_keys"] == 200
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=len(values), units_cap=10 ** 4)
    assert rc == N.GX_OK and totals["n_keys"] == 200
    got = check(gorp, data, offsets, ids, caps, parts, max_keys=1, key_units_cap=1)
    assert got["totals"]["n_keys"] == 200 and got["lines"].tolist() == [2] * 200


def test_more_keys_in_a_workgroup_than_its_lds_table_holds():
    gorp = trivial_handle(2)
    assert 8 <= LDS_KEYS < 128
    rng = np.random.default_rng(31)
    distinct = LDS_KEYS + 1
    block = [b"%d" % (1000 + j) for j in range(distinct)]
    block = block + [block[j] for j in rng.integers(0, distinct, 256 - distinct)]       # 256 consecutive lines, every key at least once, most repeated
    assert len(block) == 256 and len(set(block)) == distinct
    values = []
    for rep in range(9):                                                               # the same keys from several workgroups
        order = rng.permutation(256)
        values += [block[j] for j in order]
    values += [b"1000"] * 100
    data, offsets, ids, caps = values_batch(values, rng.integers(0, 2, len(values)))
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0, 0)])
    assert got["totals"]["n_keys"] == distinct and sum(got["lines"]) == len(values)
    assert sum(s["sum"] for s in got["stats"]) == sum(int(v) for v in values)
    # twice as many again: most slots add to global memory directly
    more = [b"%d" % (5000 + j) for j in range(3 * LDS_KEYS)] * 3
    data, offsets, ids, caps = values_batch(values + more, np.zeros(len(values) + len(more)))
    assert check(gorp, data, offsets, ids, caps, [(0, 0, 0)])["totals"]["n_keys"] == distinct + 3 * LDS_KEYS


# ---------------------------------------------------------------------------
# the numbers per key
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u8"])
def test_integer_table_over_three_keys(fmt):
    gorp = trivial_handle(2, groups=2)
    lines, caps, ids = [], [], []
    for rep, key in enumerate([b"k0", b"key1", b""] * 2):
        for v in INT_TABLE:
            lines.append(key + v + b"9")
            caps.append([0, len(key), len(key), len(key) + len(v)])
            ids.append(rep % 2)
        lines.append(key + b"5")
        caps.append([0, len(key), -1, -1])                     # a key whose number is unset
        ids.append(rep % 2)
    data, offsets = csr(lines)
    ids, caps = np.array(ids, np.int32), np.array(caps, np.int32)
    id_col, rows = in_format(ids, caps, fmt)
    got = check(gorp, data, offsets, id_col, rows, [(0, 0, 1), (1, 0, 1)])
    assert len(got["stats"]) == 3 and all(s["numbers"] == 2 * 7 and s["not_numbers"] == 2 * 9 and s["unset"] == 2 for s in got["stats"])
    assert all(s["min"] == INT64_MIN and s["max"] == INT64_MAX for s in got["stats"])
    # a part that only counts beside one that measures: the key's lines of the first add nothing to its numbers
    got = check(gorp, data, offsets, id_col, rows, [(0, 0), (1, 0, 1)])
    assert all(s["lines"] == 17 for s in got["stats"]) and got["lines"].tolist() == [34, 34, 34]
    # a key with no number at all
    got = check(gorp, data, offsets, id_col, rows, [(0, 0, 0)])
    assert [(s["numbers"], s["min"], s["max"], s["sum"]) for s in got["stats"]] == [(0, None, None, 0)] * 3


@pytest.mark.parametrize("name", ["up", "down", "mixed"])
def test_128_bit_sums_over_three_keys(name):
    gorp = trivial_handle(1, groups=2)
    numbers = [str(v).encode() for count, v in SUM_SEQUENCES[name] for _ in range(count)]
    assert len(numbers) == 70000
    rng = np.random.default_rng(3)
    rng.shuffle(numbers)
    which = rng.integers(0, 3, len(numbers))
    keys = [b"a", b"bb", b"a" * 21]
    lines = [keys[w] + v for w, v in zip(which, numbers)]
    data, offsets = csr(lines)
    caps = np.array([[0, len(keys[w]), len(keys[w]), len(ln)] for w, ln in zip(which, lines)], np.int32)
    got = check(gorp, data, offsets, np.zeros(len(lines), np.int32), caps, [(0, 0, 1)])
    assert sum(s["sum"] for s in got["stats"]) == sum(int(v) for v in numbers) and len(got["stats"]) == 3
    assert any(not INT64_MIN <= s["sum"] <= INT64_MAX for s in got["stats"])


# ---------------------------------------------------------------------------
# code units: UTF-16, UTF-8 bytes
# ---------------------------------------------------------------------------
def test_utf16_units_and_a_value_that_is_not_ascii():
    gorp = trivial_handle(2)
    lines = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31], [0x3100], [0xFF11], [], [0x416, 0x16], [0x16, 0x416], [0xFF11, 0x31], [0x0031, 0x0000], []]
    data, offsets = csr(lines * 2, dtype=np.uint16)
    ids = np.array([0] * len(lines) + [1] * len(lines), np.int32)
    caps = np.array([[0, len(ln)] for ln in lines * 2], np.int32)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 0), (1, 0)])
    assert got["totals"]["n_keys"] == 9 and got["lines"].tolist()[:2] == [4, 4] and got["key_units"].dtype == np.uint16
    assert (got["stats"][0]["numbers"], got["stats"][1]["not_numbers"], got["stats"][1]["numbers"]) == (2, 2, 0)       # U+FF11 is a key, and no number
    listed = gorp.group_lines(data, offsets, ids, caps, [(0, 0), (1, 0)])
    assert listed["keys"][:3] == ["1", "１", "1１"] and "" in listed["keys"]
    for fmt in ("u16", "u8"):
        id_col, _ = in_format(ids, caps, fmt)
        assert plain(check(gorp, data, offsets, id_col, None, [(0, 0, 0), (1, 0)])) == plain(got)
    got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], where=[(1, 0, "contains", "１")])
    assert got["totals"]["lines"] == len(lines) + 4
    # lines of the README definition as UTF-16
    gorp = Gorp.construct(W.readme3_definition())
    n = 600
    t_data, _, _ = W.readme3_lines(n, seed=8)
    data = t_data.numpy().astype(np.uint16)
    data[np.flatnonzero(data == ord("~"))[::3]] = 0x416
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert len(check(gorp, data, offsets, ids, caps, VERB_PARTS)["lines"]) == 6
    assert check(gorp, data, offsets, ids, caps, [("GetRequest", "path")])["totals"]["n_keys"] > 100


def test_utf8_bytes_with_a_key_that_is_not_ascii():
    gorp = Gorp.construct(W.readme3_definition())
    rng = random.Random(12)
    lines = []
    for j in range(1500):
        verb = rng.choice(["GET", "GET", "PUT", "POST"])
        lines.append("[%d]: %s %dms /%s%s" % (rng.randrange(1, 10 ** 9), verb, rng.choice([7, 499, 500, rng.randrange(0, 100000)]), rng.choice(["v1/", "café/", "Ж€/"]),
                                              "x" * rng.randrange(0, 4)))
    data, offsets = lines_to_csr([ln.encode("utf-8") for ln in lines])
    assert (data >= 0x80).any()
    ids, caps = gorp.extract_batch(data, offsets, utf8="bytes")
    parts = [("GetRequest", "path", "timeTakenInMsec"), ("PutRequest", "path", "timeTakenInMsec"), ("OtherRequest", "path")]
    got = check(gorp, data, offsets, ids, caps, parts, utf8="bytes")
    assert got["totals"]["n_keys"] == 12 and got["totals"]["keyed"] == 1500
    listed = gorp.group_lines(data, offsets, ids, caps, parts, utf8="bytes")
    assert "/café/" in listed["keys"] and "/Ж€/xxx" in listed["keys"] and all(isinstance(k, str) for k in listed["keys"])
    got = check(gorp, data, offsets, ids, caps, parts, where=[("GetRequest", "path", "contains", "café")], utf8="bytes")
    assert got["totals"]["lines"] < 1500
    # utf8 = 2 (offsets in units over a byte buffer) and no_sync are refused on a handle with a device too
    rc, _, arrays = raw_call(gorp, data, offsets, ids, caps, parts, utf8=2)
    assert rc == N.GX_E_ARG and "utf8" in N.last_error() and untouched(arrays)
    rc, _, arrays = raw_call(gorp, data, offsets, ids, caps, parts, no_sync=1)
    assert rc == N.GX_E_ARG and "no_sync" in N.last_error() and untouched(arrays)


# ---------------------------------------------------------------------------
# device buffers: alignment, the end of the allocation, poison around key_units, stream order, determinism
# ---------------------------------------------------------------------------
def on_device(gorp, data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, max_keys, units_cap, values=True, dtype=None, line_key=True, **kw):
    """group_lines_device with torch buffers; key_units sits between two fences of poison.  Returns (rc, totals, dict of host arrays)."""
    import torch
    dtype = dtype or torch.uint8
    fence = 64
    units = torch.full((fence + units_cap + fence,), 0x5A, dtype=dtype, device="cuda")
    koff = torch.full((max_keys + 1 + 4,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((max_keys + 4,), -1, dtype=torch.int32, device="cuda")
    lines = torch.full((max_keys + 4,), -1, dtype=torch.int64, device="cuda")
    stats = torch.full((max_keys + 4, 8), -1, dtype=torch.int64, device="cuda")
    lkey = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc, totals = gorp.group_lines_device(data_ptr, off_ptr, n, ids_ptr, caps_ptr, parts, key_units_ptr=units.data_ptr() + fence * units.element_size(),
                                         key_units_cap=units_cap, key_offsets_ptr=koff.data_ptr(), key_first_line_ptr=first.data_ptr(),
                                         key_lines_ptr=lines.data_ptr(), key_stats_ptr=stats.data_ptr() if values else None,
                                         line_key_ptr=lkey.data_ptr() if line_key else None, max_keys=max_keys, **kw)
    torch.cuda.synchronize()
    k, u = (totals["n_keys"], totals["key_units"]) if rc == N.GX_OK else (0, 0)
    h_units = units.cpu().numpy()
    assert (h_units[:fence] == 0x5A).all() and (h_units[fence + u:] == 0x5A).all()                       # nothing outside [0, key_units)
    assert (koff[k + 1:] == -1).all() and (first[k:] == -1).all() and (lines[k:] == -1).all() and (stats[k:] == -1).all() and (lkey[n:] == 0x5A5A5A5A).all()
    if rc != N.GX_OK:
        assert (koff == -1).all() and (lkey == 0x5A5A5A5A).all()
    return rc, totals, {"key_units": h_units[fence:fence + u], "key_offsets": koff[:k + 1].cpu().numpy().view(np.uint32), "first_line": first[:k].cpu().numpy().view(np.uint32),
                        "lines": lines[:k].cpu().numpy().view(np.uint64), "stats": stats[:k].cpu().numpy(), "line_key": lkey[:n].cpu().numpy().view(np.uint32)}


def stats_rows(stats):
    """Gorp.group_lines' stats dicts as the eight words of gx_measure_stats"""
    out = []
    for s in stats:
        total = s["sum"]
        out.append([s["lines"], s["numbers"], s["unset"], s["not_numbers"], INT64_MAX if s["min"] is None else s["min"], INT64_MIN if s["max"] is None else s["max"],
                    (total & (2 ** 64 - 1)) - (2 ** 64 if total & 2 ** 63 else 0), total >> 64])
    return np.array(out, np.int64).reshape(len(stats), 8)


def same_arrays(dev, host):
    for k in ("key_units", "key_offsets", "first_line", "lines", "line_key"):
        assert np.array_equal(dev[k], host[k]), k
    if host["stats"] is not None:
        assert np.array_equal(dev["stats"], stats_rows(host["stats"]))


def test_device_buffers_at_every_misalignment_end_with_the_last_capture():
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n = 3000
    pool = [str(int(v)).encode() for v in rng.integers(-10 ** 6, 10 ** 12, 150)]
    values = [pool[j] for j in rng.integers(0, 150, n)]
    values[-1] = b"9223372036854775807"                                       # a new key: the last capture ends at the buffer's last byte
    data, offsets, ids, caps = values_batch(values, rng.integers(-2, 4, n))
    ids[-1] = 3
    rows8 = pack(ids, caps, np.uint8)
    parts = [(3, 0, 0), (0, 0, 0), (1, 0)]
    host = check(gorp, data, offsets, ids, caps, parts)
    assert plain(check(gorp, data, offsets, rows8, None, parts)) == plain(host) and host["stats"][-1]["max"] == INT64_MAX and host["lines"][-1] == 1
    k, units = host["totals"]["n_keys"], host["totals"]["key_units"]
    d_off, d_ids, d_caps = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    for mis in range(16):
        src = torch.empty(mis + len(data), dtype=torch.uint8, device="cuda")     # sized exactly: the batch ends where the tensor ends
        src[mis:] = torch.from_numpy(data).cuda()
        rc, totals, dev = on_device(gorp, src.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), parts, k, units)
        assert rc == N.GX_OK and totals == host["totals"]
        same_arrays(dev, host)
        d_rows = torch.empty(mis + rows8.size, dtype=torch.uint8, device="cuda")
        d_rows[mis:] = torch.from_numpy(rows8.reshape(-1)).cuda()
        rc, totals, dev = on_device(gorp, src.data_ptr() + mis, d_off.data_ptr(), n, d_rows.data_ptr() + mis, None, parts, k + mis, units + mis, compact=2,
                                    where=[(3, 0, ">=", -10 ** 7)])
        assert rc == N.GX_OK
        same_arrays(dev, host)
    # too small on the device: nothing written (on_device looks at every buffer)
    rc, totals, dev = on_device(gorp, src.data_ptr() + 15, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), parts, k, units - 1)
    assert rc == N.GX_E_LIMIT and totals == host["totals"]
    rc, totals, dev = on_device(gorp, src.data_ptr() + 15, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), parts, k - 1, units)
    assert rc == N.GX_E_LIMIT and totals == host["totals"]
    # dense ids without capture rows: refused on a handle with a device too
    with pytest.raises(GorpError) as ei:
        gorp.group_lines_device(src.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), None, parts)
    assert ei.value.code == N.GX_E_ARG


@pytest.mark.parametrize("K", [1, 32, 2048])
def test_extraction_counts_parts_on_the_first_and_the_last(K):
    gorp = trivial_handle(K)
    rng = np.random.default_rng(K)
    n = 6000
    pool = [b"%x" % (j * 7919) for j in range(70)]
    values = [pool[j] for j in rng.integers(0, 70, n)]
    others = np.array(sorted({0, K // 2, K - 1, 1 % K, -1, -2, -1 - K, K}), np.int32)
    data, offsets, ids, caps = values_batch(values, rng.choice(others, n))
    caps[rng.random(n) < 0.1] = -1
    parts = [(k, 0, 0) for k in sorted({0, K - 1})]
    got = check(gorp, data, offsets, ids, caps, parts)
    assert got["totals"]["n_keys"] == 70 and got["totals"]["unset"] > 30 and got["totals"]["lines"] == np.isin(ids, [0, K - 1]).sum()


def test_64_parts_at_once():
    gorp = trivial_handle(70, groups=2)
    rng = np.random.default_rng(64)
    n = 5000
    pool = [b"%d" % j for j in range(90)]
    values = [pool[j] for j in rng.integers(0, 90, n)]
    data, offsets = csr(values)
    caps = np.array([[0, len(v), 1, len(v)] for v in values], np.int32)         # group 1: the value without its first unit
    ids = rng.integers(-2, 70, n).astype(np.int32)
    parts = [(k, k % 2, (k + 1) % 2 if k % 3 else None) for k in range(69, 5, -1)]
    assert len(parts) == 64
    got = check(gorp, data, offsets, ids, caps, parts)
    assert got["totals"]["lines"] == (ids >= 6).sum() and got["totals"]["n_keys"] > 90        # "12" and "2" are keys of different groups' values


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
    batch = (data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None)
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True, compact=2,
                                  line_bytes_hint=L)
        rc, totals, got = on_device(gorp, *batch, VERB_PARTS, 6, 40, where=where, compact=2, stream=stream.cuda_stream)
        rc2, totals2, again = on_device(gorp, *batch, VERB_PARTS, 6, 40, where=where, compact=2, stream=stream.cuda_stream)
    stream.synchronize()
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(unpack(h_rows)[0], cat.cpu().numpy().astype(np.int32))
    host = check(gorp, h_data, h_off, h_rows, None, VERB_PARTS, where=where)
    assert rc == rc2 == N.GX_OK and totals == totals2 == host["totals"] and totals["n_keys"] == 6
    same_arrays(got, host)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k                              # two runs: the same bits
    # the path as key: tens of thousands of keys, claimed by whichever lane came first, delivered the same
    by_path = [("GetRequest", "path", "timeTakenInMsec"), ("PutRequest", "path", "timeTakenInMsec"), ("OtherRequest", "path", "timeTakenInMsec")]
    rc, totals, a = on_device(gorp, *batch, by_path, n, n * L, compact=2)
    assert rc == N.GX_OK and totals["n_keys"] > n // 2
    for _ in range(2):
        rc, totals2, b = on_device(gorp, *batch, by_path, n, n * L, compact=2)
        assert totals2 == totals and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_offsets_on_the_device_that_go_backwards_are_refused_by_the_build_pass():
    import torch
    gorp = trivial_handle(1)
    data = torch.from_numpy(np.frombuffer(b"123" + b"\0" * 13, np.uint8).copy()).cuda()
    ids = torch.zeros(3, dtype=torch.int32, device="cuda")
    caps = torch.tensor([[0, 1]] * 3, dtype=torch.int32, device="cuda")
    lkey = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for dtype, offsets64 in ((torch.int64, True), (torch.int32, False)):
        d_off = torch.tensor([0, 2, 1, 3], dtype=dtype, device="cuda")          # line 1 has 2^64 - 1 (2^32 - 1 + the wrap) units: nothing of it is read
        with pytest.raises(GorpError) as ei:
            gorp.group_lines_device(data.data_ptr(), d_off.data_ptr(), 3, ids.data_ptr(), caps.data_ptr(), [(0, 0, 0)], line_key_ptr=lkey.data_ptr(),
                                    max_keys=3, offsets64=offsets64)
        torch.cuda.synchronize()
        assert ei.value.code == N.GX_E_LIMIT and "4 G" in ei.value.message and (lkey == 0x5A5A5A5A).all()
    d_off = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    rc, totals = gorp.group_lines_device(data.data_ptr(), d_off.data_ptr(), 3, ids.data_ptr(), caps.data_ptr(), [(0, 0, 0)], line_key_ptr=lkey.data_ptr(), max_keys=3)
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["n_keys"] == 3 and lkey.tolist() == [0, 1, 2]


def test_a_whole_file_call_with_device_outputs_is_done_when_it_returns():
    """Its emit pass reads the lines' offsets, ids and capture rows from the handle's buffers, which the next whole-file call -- here on
    another stream, with another text -- overwrites."""
    import torch
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    text = "".join("[%d]: GET %dms /some/long/path/number/%d/of/many\n" % (j, j % 50, j % 5000) for j in range(60000)).encode()
    other = "".join("[%d]: PUT %dms /x%d\n" % (j, j, j) for j in range(90000)).encode()
    parts = [("GetRequest", "path", "timeTakenInMsec")]
    want, _, n_lines = gorp.text_group_lines(text, parts, keys="csr")
    k, units = want["totals"]["n_keys"], want["totals"]["key_units"]
    assert k == 5000 and n_lines == 60000
    pad = lambda b: torch.from_numpy(np.frombuffer(b + b"\0" * 16, np.uint8).copy()).cuda()
    d_text, d_other = pad(text), pad(other)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        d_units = torch.zeros(units, dtype=torch.uint8, device="cuda")
        d_koff = torch.zeros(k + 1, dtype=torch.int32, device="cuda")
        d_lines = torch.zeros(k, dtype=torch.int64, device="cuda")
        d_lkey = torch.zeros(n_lines, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc, totals, _, nl = gorp.text_group_lines_device(d_text.data_ptr(), len(text), parts, key_units_ptr=d_units.data_ptr(), key_units_cap=units,
                                                         key_offsets_ptr=d_koff.data_ptr(), key_lines_ptr=d_lines.data_ptr(), line_key_ptr=d_lkey.data_ptr(),
                                                         max_keys=k, stream=s1.cuda_stream)
        # no wait on s1 here: the outputs are complete, and the next call may take the handle's buffers
        got = (d_units.cpu().numpy().copy(), d_koff.cpu().numpy().view(np.uint32).copy(), d_lines.cpu().numpy().view(np.uint64).copy())
        gorp.text_capture_stats_device(d_other.data_ptr(), len(other), [("PutRequest", "timeTakenInMsec")], stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert rc == N.GX_OK and totals == want["totals"] and nl == n_lines
        assert np.array_equal(got[0], want["key_units"]) and np.array_equal(got[1], want["key_offsets"]) and np.array_equal(got[2], want["lines"])
        assert np.array_equal(d_units.cpu().numpy(), want["key_units"]) and np.array_equal(d_lkey.cpu().numpy().view(np.uint32), want["line_key"])


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------
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
        elif r < 0.14:
            line = line + "\x0bq"                                   # the automaton takes VT for \S, the capture regexp does not: the line raises
        elif r < 0.17:
            line = ""
        out.append(line)
    return out


@pytest.mark.parametrize("utf8", [False, True])
def test_text_group_lines_is_split_extract_group(utf8):
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in text_lines(3000, 21, utf8)]
    text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 777ms /tail"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
    assert (ids < -1).sum() > 50 and (ids == -1).sum() > 100
    by_path = [("GetRequest", "path", "timeTakenInMsec"), ("PutRequest", "path", "timeTakenInMsec"), ("OtherRequest", "path")]
    wheres = [None, [("GetRequest", "timeTakenInMsec", ">=", 500)], [("GetRequest", "path", "contains", "café" if utf8 else "/v1/"), ("PutRequest", "timeTakenInMsec", "<", 500)]]
    for parts in (VERB_PARTS, by_path):
        for where in wheres:
            want = check(gorp, data, offsets, ids, caps, parts, where=where, utf8="bytes" if utf8 else None)
            got, counts, n_lines = gorp.text_group_lines(text, parts, where=where, utf8=utf8, keys="csr")
            assert plain(got) == plain(want) and n_lines == len(raw) + 1 == len(got["line_key"])
            assert np.array_equal(counts, gorp.count_outcomes(ids))
    listed, _, _ = gorp.text_group_lines(text, by_path, utf8=utf8)
    assert (("/café/" in listed["keys"]) if utf8 else (b"/api/v1/x" in listed["keys"])) and listed["keys"][-1] == ("/tail" if utf8 else b"/tail")
    # no parts: counts and the line count alone; an empty text
    got, counts, n_lines = gorp.text_group_lines(text, [], utf8=utf8)
    assert got["keys"] == [] and n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids)) and (got["line_key"] == NONE).all()
    got, counts, n_lines = gorp.text_group_lines(b"", VERB_PARTS, utf8=utf8)
    assert n_lines == 0 and counts.sum() == 0 and got["keys"] == [] and got["totals"]["lines"] == 0 and got["stats"] == []


# ---------------------------------------------------------------------------
# a batch that lives on the device, against torch.unique
# ---------------------------------------------------------------------------
def test_200k_lines_on_the_device_against_torch_unique():
    import torch
    gorp = trivial_handle(2)
    n, w = 200000, 6
    g = torch.Generator(device="cuda").manual_seed(5)
    number = torch.randint(0, 1000, (n,), device="cuda", generator=g)           # the line's value number ...
    spelled = number * 899 + 100000                                             # ... spelled with six digits (at most 998101), distinct per number
    digits = ((spelled[:, None] // (10 ** torch.arange(w - 1, -1, -1, device="cuda"))[None, :]) % 10 + 48).to(torch.uint8).contiguous()
    d_off = (torch.arange(n + 1, device="cuda") * w).to(torch.int32)
    ids = torch.randint(-1, 2, (n,), device="cuda", generator=g).to(torch.int32)
    caps = torch.tensor([0, w], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
    rc, totals, got = on_device(gorp, digits.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), [(0, 0, 0), (1, 0)], 1000, 6000)
    assert rc == N.GX_OK and totals["n_keys"] == 1000 and totals["key_units"] == 6000
    counted = ids >= 0
    uniq, inverse, count = torch.unique(number[counted], return_inverse=True, return_counts=True)
    # torch's keys are sorted by value; reorder by first appearance
    at = torch.arange(int(counted.sum()), device="cuda")
    first_at = torch.full((len(uniq),), n, device="cuda").scatter_reduce(0, inverse, at, "amin")
    order = torch.argsort(first_at)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(len(order), device="cuda")
    want_key = torch.full((n,), NONE, dtype=torch.int64, device="cuda")
    want_key[counted] = rank[inverse]
    assert np.array_equal(got["line_key"].astype(np.int64), want_key.cpu().numpy())
    assert np.array_equal(got["lines"].astype(np.int64), count[order].cpu().numpy())
    assert np.array_equal(got["first_line"].astype(np.int64), torch.nonzero(counted).flatten()[first_at[order]].cpu().numpy())
    spelled_keys = np.array([int(bytes(got["key_units"][6 * j:6 * j + 6])) for j in range(1000)])
    assert np.array_equal(spelled_keys, (uniq[order] * 899 + 100000).cpu().numpy())
    # the numbers of extraction 0's lines, per key
    zero = ids == 0
    sums = torch.zeros(len(uniq), dtype=torch.int64, device="cuda").scatter_add(0, inverse[zero[counted]], spelled[counted][zero[counted]])
    assert np.array_equal(got["stats"][:, 6], sums[order].cpu().numpy()) and (got["stats"][:, 7] == 0).all()
    assert np.array_equal(got["stats"][:, 0], torch.bincount(inverse[zero[counted]], minlength=len(uniq))[order].cpu().numpy())
