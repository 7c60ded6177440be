"""GPU tests of gx_bucket_lines / gx_text_bucket_lines: the lines of a batch counted and measured per interval of a number they captured
-- the occupied buckets in ascending order of their number, the first line, the lines and the stats of every bucket, the bucket of every
line.

Expected values come from tests/bucket_oracle.py -- where_oracle / number_oracle for which lines count and what their number is, Python's
// on unbounded ints for the bucket, a dict sorted by key -- and everything is compared bit for bit.  Every case runs once more under
GX_BUCKET_ALL_DIGITS and (up to 4 096 buckets) under GX_GROUP_WEAK_HASH and must give the same bytes.  Most batches are fabricated against
handles of K identical, trivial extractions with two groups: a line is its number's text, its value's text and filler, its capture row
made up here; the end-to-end case takes ids and rows from gx_extract_batch.  The large shape is compared with a numpy restatement
(np.unique on (v - origin) // width), which tests/test_bucket_host.py compares with the oracle on smaller draws of the same generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, parse_number
from bucket_oracle import INT64_MAX, INT64_MIN, NONE, batch, bucket_lines, decode_parts, digits_batch, draw, np_buckets, same
from number_oracle import KINDS
from stats_oracle import SUM_SEQUENCES
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_bucket.hpp")).read()
WG_LINES = int(re.search(r"constexpr uint32_t BUCKET_WG_LINES = (\d+);", RULE).group(1))      # the lines a workgroup of the build pass covers
LDS_KEYS = int(re.search(r"GROUP_LDS_KEYS = (\d+);", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_group.hpp")).read()).group(1))
BLOCK = 2048                                                                                  # gx_scan.hpp: SCAN_THREADS x SCAN_ITEMS
P0 = [(0, 0)]
P0V = [(0, 0, 1)]
FIELDS = ("bucket_number", "first_line", "lines", "line_bucket")


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, width, origin=0, where=None, utf8=None, formats=None, **kw):
    """bucket_lines against the restatement, every field; then under the test hooks, the same bytes.  Returns what the call returned."""
    p = gorp.bucket_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    fm = {key: (KINDS[kind], scale) for key, (kind, scale) in (formats or {}).items()}
    want = bucket_lines(data, offsets, ids, caps, decode_parts(p), gorp._bucket_origin(p, origin), width, decode_terms(terms), gorp.num_extractions, fm)
    got = gorp.bucket_lines(data, offsets, ids, caps, p, width, origin, where=terms, utf8=utf8, **kw)
    same(got, want)
    hooks = [dict(all_digits=True)] + ([dict(weak_hash=True), dict(weak_hash=True, all_digits=True)] if want["totals"]["n_buckets"] <= 4096 else [])
    for hook in hooks:
        again = gorp.bucket_lines(data, offsets, ids, caps, p, width, origin, where=terms, utf8=utf8, **dict(kw, **hook))
        assert again["totals"] == got["totals"] and again["stats"] == got["stats"], hook
        for name in FIELDS:
            assert again[name].dtype == got[name].dtype and again[name].tobytes() == got[name].tobytes(), (hook, name)
    return got


_handles = {}


def trivial_handle(K, groups=2, tag=""):
    """K identical extractions `a(.*)(.*)`: a handle for ids and capture rows made up here (tag: a handle of its own, for number formats)."""
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


# ---------------------------------------------------------------------------
# what a bucket is
# ---------------------------------------------------------------------------
def test_four_lines_around_the_origin():
    gorp = trivial_handle(1)
    got = check(gorp, *batch([-1, 0, -60_000, -60_001]), P0, 60_000)
    assert got["bucket_number"].tolist() == [-2, -1, 0] and got["lines"].tolist() == [1, 2, 1] and got["line_bucket"].tolist() == [1, 2, 1, 0]
    got = check(gorp, *batch([999, 1000, 940, 939]), P0, 60, origin=1000)                  # the same four around another origin
    assert got["bucket_number"].tolist() == [-2, -1, 0] and got["first_line"].tolist() == [3, 0, 1]
    t = got["totals"]
    assert (t["first_bucket"], t["last_bucket"], t["n_buckets"], t["bucketed"]) == (-2, 0, 3, 4)


def test_width_one_and_width_int64_max():
    gorp = trivial_handle(1)
    numbers = [INT64_MIN, INT64_MIN + 1, -2, -1, 0, 1, INT64_MAX - 1, INT64_MAX, -1, INT64_MAX]
    got = check(gorp, *batch(numbers), P0, 1)
    assert got["totals"]["out_of_range"] == 1 and got["bucket_number"].tolist() == [INT64_MIN + 1, -2, -1, 0, 1, INT64_MAX - 1, INT64_MAX]
    got = check(gorp, *batch(numbers), P0, INT64_MAX)
    assert got["bucket_number"].tolist() == [-2, -1, 0, 1] and got["lines"].tolist() == [1, 4, 3, 2] and got["totals"]["out_of_range"] == 0
    got = check(gorp, *batch(numbers), P0, 1, origin=INT64_MIN)                             # v - origin needs 65 bits: exact all the same
    assert got["bucket_number"].tolist() == [0, 1, INT64_MAX - 1, INT64_MAX] and got["totals"]["out_of_range"] == 5 and got["lines"].tolist() == [1, 1, 1, 2]
    got = check(gorp, *batch(numbers), P0, 2, origin=INT64_MAX)
    assert got["bucket_number"][0] == -INT64_MAX and got["bucket_number"][-1] == 0 and got["totals"]["out_of_range"] == 1


def test_the_four_classes_add_up():
    gorp = trivial_handle(2)
    numbers = [5, INT64_MIN, None, b"x", 7, b"", b"9223372036854775808", 6, 5]
    data, offsets, ids, caps = batch(numbers, lengths=[4] * 9, ids=[0, 0, 0, 0, 1, 0, 0, -1, -2])
    got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], 1)
    t = got["totals"]
    assert (t["lines"], t["bucketed"], t["unset"], t["not_numbers"], t["out_of_range"]) == (7, 2, 1, 3, 1)
    assert got["line_bucket"].tolist() == [0, NONE, NONE, NONE, 1, NONE, NONE, NONE, NONE]
    # a part for extraction 0 alone: extraction 1's line does not count
    assert check(gorp, data, offsets, ids, caps, P0, 1)["totals"]["lines"] == 6
    # no part at all, and no line at all: all zeros, no line has a bucket
    got = check(gorp, data, offsets, ids, caps, [], 1)
    assert got["totals"]["lines"] == 0 and got["totals"]["n_buckets"] == 0 and set(got["line_bucket"].tolist()) == {NONE} and got["totals"]["exact"]
    got = check(gorp, *batch([]), P0, 1)
    assert got["totals"]["n_buckets"] == 0 and len(got["line_bucket"]) == 0
    got = check(gorp, *batch([None, b"x"]), P0, 1)                                            # lines, none of them bucketed
    assert got["totals"]["n_buckets"] == 0 and got["totals"]["lines"] == 2 and got["line_bucket"].tolist() == [NONE, NONE]


def test_buckets_leave_ascending_whatever_the_order_of_the_lines():
    gorp = trivial_handle(1)
    numbers = list(range(900, -900, -7))
    got = check(gorp, *batch(numbers), P0, 10)
    assert (np.diff(got["bucket_number"]) > 0).all() and (np.diff(got["first_line"].astype(np.int64)) < 0).all()
    assert got["bucket_number"][0] < 0 < got["bucket_number"][-1]
    rng = np.random.default_rng(8)
    got = check(gorp, *batch(rng.integers(-10 ** 6, 10 ** 6, 3000).tolist()), P0, 1000)
    first = got["first_line"].astype(np.int64)
    assert (np.diff(first) < 0).any() and (np.diff(first) > 0).any()


# ---------------------------------------------------------------------------
# contention and the workgroup's table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one bucket", "an edge inside a wave", "every line its own", "two buckets interleaved"])
def test_contention(shape):
    gorp = trivial_handle(1)
    n = 3 * WG_LINES
    i = np.arange(n)
    numbers = {"one bucket": 600 + i % 60, "an edge inside a wave": np.where(i % 64 <= 30, 600, 660) + i % 7, "every line its own": 60 * (n - i),
               "two buckets interleaved": 600 + 60 * (i & 1)}[shape]
    got = check(gorp, *batch(numbers.tolist(), values=(i % 1000).tolist()), P0V, 60)
    assert got["totals"]["n_buckets"] == {"one bucket": 1, "an edge inside a wave": 2, "every line its own": n, "two buckets interleaved": 2}[shape]
    assert int(got["lines"].sum()) == n and sum(s["numbers"] for s in got["stats"]) == n
    if shape == "an edge inside a wave":
        assert got["first_line"].tolist() == [0, 31] and got["lines"].tolist() == [31 * 12, 33 * 12]


@pytest.mark.parametrize("distinct", [LDS_KEYS + 1, 2 * LDS_KEYS + 1])
def test_more_buckets_in_a_workgroup_than_its_lds_table_claims(distinct):
    gorp = trivial_handle(1)
    assert distinct <= WG_LINES
    rng = np.random.default_rng(distinct)
    block = np.concatenate([np.arange(distinct), rng.integers(0, distinct, WG_LINES - distinct)])    # one workgroup's lines: every bucket at least once
    numbers = np.concatenate([rng.permutation(block), rng.permutation(block) + 3, rng.permutation(block)[:100]]) * 10
    got = check(gorp, *batch(numbers.tolist(), values=(numbers % 97).tolist()), P0V, 10)
    assert got["totals"]["n_buckets"] == distinct + 3 and int(got["lines"].sum()) == len(numbers)


@pytest.mark.parametrize("n_buckets", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_bucket_counts_at_the_edges_of_a_scan_and_a_sort_block(n_buckets):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n_buckets)
    numbers = rng.permutation(np.concatenate([np.arange(n_buckets), rng.integers(0, n_buckets, 500)])) * 3 - 2000
    got = check(gorp, *batch(numbers.tolist()), P0, 3, max_buckets=n_buckets)
    assert got["totals"]["n_buckets"] == n_buckets and int(got["lines"].sum()) == n_buckets + 500


def test_one_line():
    gorp = trivial_handle(1)
    got = check(gorp, *batch([-7], values=[3]), P0V, 2)
    assert got["bucket_number"].tolist() == [-4] and got["stats"][0]["sum"] == 3 and got["totals"]["first_bucket"] == got["totals"]["last_bucket"] == -4


@pytest.mark.parametrize("buckets", [(0, 1), (0, 64), (-1, 0), (0, 2 ** 62), (5, 5), (INT64_MIN + 1, INT64_MAX), (63, 64, 4095, 4096)])
def test_the_digit_plan(buckets):
    gorp = trivial_handle(1)
    numbers = [buckets[q % len(buckets)] for q in (3, 1, 0, 2, 1, 0, 3, 2, 2)]
    got = check(gorp, *batch(numbers), P0, 1)
    assert got["bucket_number"].tolist() == sorted(set(buckets))


# ---------------------------------------------------------------------------
# the full table and the capacity
# ---------------------------------------------------------------------------
def raw_call(gorp, data, offsets, ids, caps, parts, width, max_buckets, want=("number", "first", "lines", "stats", "line_bucket"), poison=0xAB):
    """gx_bucket_lines itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.bucket_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n = len(offsets) - 1
    arrays = {"number": np.zeros(max_buckets + 8, np.int64), "first": np.zeros(max_buckets + 8, np.uint32), "lines": np.zeros(max_buckets + 8, np.uint64),
              "stats": np.zeros((max_buckets + 8) * 64, np.uint8), "line_bucket": np.zeros(n + 8, np.uint32)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_bucket_out(ptr("number"), ptr("first"), ptr("lines"), ptr("stats") if p.has_values else None, ptr("line_bucket"), max_buckets)
    totals = N.gx_bucket_totals()
    rc = N.lib().gx_bucket_lines(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, 0, width, None, 0, 0,
                                 C.byref(out), C.byref(totals), C.byref(o))
    return rc, Gorp._bucket_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


def test_a_full_table_and_a_capacity_too_small():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(65)
    data, offsets, ids, caps = batch(rng.permutation(np.repeat(np.arange(65), 6)).tolist(), values=[1] * 390)
    for want in (("number", "first", "lines", "stats", "line_bucket"), ()):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0V, 1, 32, want=want)               # 64 slots, 65 buckets
        assert rc == N.GX_E_LIMIT and not totals["exact"] and totals["n_buckets"] == 65 and totals["lines"] == 390 and untouched(arrays)
        assert "slots" in N.last_error()
    data, offsets, ids, caps = batch(rng.permutation(np.repeat(np.arange(33), 6)).tolist() + [None, b"x"], values=[1] * 200)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0V, 1, 32)                              # 33 buckets fit the table, not the arrays
    assert rc == N.GX_E_LIMIT and untouched(arrays)
    assert totals == {"n_buckets": 33, "lines": 200, "bucketed": 198, "unset": 1, "not_numbers": 1, "out_of_range": 0, "exact": True, "first_bucket": 0,
                      "last_bucket": 32}
    rc, totals2, arrays = raw_call(gorp, data, offsets, ids, caps, P0V, 1, 32, want=())                    # the size query passes
    assert rc == N.GX_OK and totals2 == totals and untouched(arrays)
    rc, totals2, arrays = raw_call(gorp, data, offsets, ids, caps, P0V, 1, 32, want=("line_bucket",))      # no per-bucket array: line_bucket alone passes
    assert rc == N.GX_OK and sorted(set(arrays["line_bucket"][:200].tolist())) == list(range(33)) + [NONE]
    rc, totals2, arrays = raw_call(gorp, data, offsets, ids, caps, P0V, 1, 33)
    assert rc == N.GX_OK and totals2 == totals and arrays["number"][:33].tolist() == list(range(33)) and (arrays["number"][33:].view(np.uint8) == 0xAB).all()
    # the Python wrapper asks again with what the totals say
    assert check(gorp, data, offsets, ids, caps, P0V, 1, max_buckets=4)["totals"]["n_buckets"] == 33


# ---------------------------------------------------------------------------
# formats and readers
# ---------------------------------------------------------------------------
def mixed_batch(n=700, seed=5, **kw):
    rng = np.random.default_rng(seed)
    numbers = (np.sort(rng.integers(0, 5000, n)) + rng.integers(-40, 40, n)).tolist()
    values = rng.integers(-500, 900, n).tolist()
    for i in rng.integers(0, n, 25):
        numbers[i] = [None, b"-", b"12x"][i % 3]
    for i in rng.integers(0, n, 25):
        values[i] = [None, b"", b"1e3"][i % 3]
    ids = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n))
    return batch(numbers, values, lengths=rng.integers(0, 24, n), ids=ids, **kw)


TWO_PARTS = [(0, 0, 1), (1, 0, 1)]


@pytest.mark.parametrize("rows", [np.uint16, np.uint8])
def test_compact_result_rows(rows):
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch()
    got = check(gorp, data, offsets, pack(ids, caps, rows), None, TWO_PARTS, 100, origin=37)
    assert got["totals"]["n_buckets"] > 40 and got["totals"]["unset"] > 0 and got["totals"]["not_numbers"] > 0


def test_offsets64_utf16_and_utf8_bytes():
    gorp = trivial_handle(2)
    base = check(gorp, *mixed_batch(), TWO_PARTS, 100)
    for kw, utf8 in ((dict(offsets_dtype=np.uint64), None), (dict(dtype=np.uint16), None), (dict(dtype=np.uint16, offsets_dtype=np.uint64), None), ({}, "bytes")):
        got = check(gorp, *mixed_batch(**kw), TWO_PARTS, 100, utf8=utf8)
        assert got["totals"] == base["totals"] and got["stats"] == base["stats"] and all(got[f].tobytes() == base[f].tobytes() for f in FIELDS)


def test_two_parts_share_one_bucket_space_and_a_where_term():
    gorp = trivial_handle(3)
    data, offsets, ids, caps = batch([100, 160, 100, 221, 100, 160], values=[500, 499, 700, 800, None, 501], ids=[0, 2, 2, 0, 0, 1])
    got = check(gorp, data, offsets, ids, caps, [(2, 0, 1), (0, 0, 1)], 60)
    assert got["bucket_number"].tolist() == [1, 2, 3] and got["lines"].tolist() == [3, 1, 1] and got["stats"][0]["unset"] == 1
    # the parts the other way round in extraction 2: its lines are bucketed by their value
    got = check(gorp, data, offsets, ids, caps, [(2, 1, 0), (0, 0, 1)], 60)
    assert got["bucket_number"].tolist() == [1, 3, 8, 11]
    # status >= 500, as a term of each extraction
    where = [(0, 1, ">=", 500), (2, 1, ">=", 500)]
    got = check(gorp, data, offsets, ids, caps, [(2, 0, 1), (0, 0, 1)], 60, where=where)
    assert got["totals"]["lines"] == 3 and got["bucket_number"].tolist() == [1, 3] and got["lines"].tolist() == [2, 1]
    got = check(gorp, *mixed_batch(), TWO_PARTS, 100, where=[(0, 1, ">=", 500), (1, 1, "<", 0)])
    assert 0 < got["totals"]["lines"] < 300


@pytest.mark.parametrize("name", ["up", "down", "mixed"])
def test_128_bit_sums_that_carry(name):
    gorp = trivial_handle(1)
    values = [v for count, v in SUM_SEQUENCES[name] for _ in range(count)]
    rng = np.random.default_rng(3)
    rng.shuffle(values)
    n = len(values)
    numbers = (np.arange(n) // 30000 * 60 + rng.integers(0, 60, n)).tolist()             # three buckets, time-ordered
    data, offsets, ids, caps = batch(numbers, values)
    p = gorp.bucket_parts(P0V)
    want = bucket_lines(data, offsets, ids, caps, decode_parts(p), 0, 60, [], 1)
    for hook in ({}, dict(weak_hash=True)):
        same(gorp.bucket_lines(data, offsets, ids, caps, p, 60, **hook), want)
    assert len(want["stats"]) == 3 and any(not -2 ** 63 <= s["sum"] < 2 ** 63 for s in want["stats"])


@pytest.fixture
def new_stream():
    """A stream of the test's own, created and destroyed here, not drawn from torch's pool (a stream taken from the pool here would shift which pool stream every later test gets)."""
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


def test_device_pointers_on_a_side_stream_and_two_runs_are_the_same_bits(new_stream):
    import torch
    gorp = trivial_handle(2)
    data, offsets, ids, caps = mixed_batch(n=5000, seed=9)
    host = check(gorp, data, offsets, ids, caps, TWO_PARTS, 100, max_buckets=256)
    k, n = host["totals"]["n_buckets"], len(ids)
    dev = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    d_data, d_off, d_ids, d_caps = dev(data), dev(offsets), dev(ids), dev(caps)
    stream = new_stream()
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        out = {"number": torch.full((k + 4,), 0x5A, dtype=torch.int64, device="cuda"), "first": torch.full((k + 4,), 0x5A, dtype=torch.int32, device="cuda"),
               "lines": torch.full((k + 4,), 0x5A, dtype=torch.int64, device="cuda"), "stats": torch.full(((k + 4) * 8,), 0x5A, dtype=torch.int64, device="cuda"),
               "line_bucket": torch.full((n + 4,), 0x5A, dtype=torch.int32, device="cuda")}
        with torch.cuda.stream(stream):
            rc, totals = gorp.bucket_lines_device(d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), TWO_PARTS, 100,
                                                  bucket_number_ptr=out["number"].data_ptr(), bucket_first_line_ptr=out["first"].data_ptr(),
                                                  bucket_lines_ptr=out["lines"].data_ptr(), bucket_stats_ptr=out["stats"].data_ptr(),
                                                  line_bucket_ptr=out["line_bucket"].data_ptr(), max_buckets=k, stream=stream.cuda_stream)
        stream.synchronize()
        assert rc == N.GX_OK and totals == host["totals"]
        runs.append({name: t.cpu().numpy() for name, t in out.items()})
    a, b = runs
    assert all(a[name].tobytes() == b[name].tobytes() for name in a)
    assert a["number"][:k].tolist() == host["bucket_number"].tolist() and a["first"][:k].view(np.uint32).tolist() == host["first_line"].tolist()
    assert a["lines"][:k].tolist() == host["lines"].tolist() and a["line_bucket"][:n].view(np.uint32).tolist() == host["line_bucket"].tolist()
    assert (a["number"][k:] == 0x5A).all() and (a["line_bucket"][n:] == 0x5A).all() and (a["stats"][8 * k:] == 0x5A).all()
    stats = a["stats"][:8 * k].reshape(k, 8)
    for j, s in enumerate(host["stats"]):
        assert stats[j, :4].tolist() == [s["lines"], s["numbers"], s["unset"], s["not_numbers"]]
        assert s["numbers"] == 0 or (int(stats[j, 4]), int(stats[j, 5])) == (s["min"], s["max"])
        assert (int(stats[j, 7]) << 64) + (int(stats[j, 6]) & (2 ** 64 - 1)) == s["sum"]


# ---------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------
def test_iso8601_milliseconds_per_minute_with_a_string_origin():
    gorp = trivial_handle(1, tag="iso")
    gorp.set_number_format(0, 0, "iso8601", 3)
    stamps = [b"2026-01-03T00:00:01.123Z", b"2026-01-03T00:00:01.124Z", b"2026-01-03T00:00:59.999Z", b"2026-01-03T00:01:00.000Z", b"2026-01-02T23:59:59.999Z",
              b"2026-01-03T01:00:00+01:00", b"2026-01-03 00:07:30,5", b"2026-01-03T00:00:60Z", b"yesterday", None, b"2026-01-04T00:00:00.000Z"]
    got = check(gorp, *batch(stamps, values=[7] * len(stamps)), P0V, 60_000, origin="2026-01-03T00:00:00Z", formats={(0, 0): ("iso8601", 3)})
    assert got["bucket_number"].tolist() == [-1, 0, 1, 7, 1440] and got["lines"].tolist() == [1, 4, 1, 1, 1]
    assert got["totals"]["not_numbers"] == 2 and got["totals"]["unset"] == 1 and got["line_bucket"][5] == 1
    assert parse_number("iso8601", 3, "2026-01-03T00:00:00Z") == 1767398400000


def test_clf_seconds_per_hour_and_decimal():
    gorp = trivial_handle(2, tag="clf")
    gorp.set_number_format(0, 0, "clf", 0)
    gorp.set_number_format(1, 0, "decimal", 2)
    gorp.set_number_format(1, 1, "decimal", 3)
    stamps = [b"03/Jan/2026:00:00:00 +0000", b"03/Jan/2026:00:59:59 +0000", b"03/Jan/2026:01:00:00 +0000", b"03/Jan/2026:01:30:00 +0100", b"02/Jan/2026:23:59:59 +0000",
              b"03/Foo/2026:00:00:00 +0000", b"0.5", b"12"]
    formats = {(0, 0): ("clf", 0), (1, 0): ("decimal", 2), (1, 1): ("decimal", 3)}
    data, offsets, ids, caps = batch(stamps, values=[1, 2, 3, 4, 5, 6, b"0.25", b"-1.0005"], ids=[0, 0, 0, 0, 0, 0, 1, 1])
    got = check(gorp, data, offsets, ids, caps, P0V, 3600, origin="03/Jan/2026:00:00:00 +0000", formats=formats)
    assert got["bucket_number"].tolist() == [-1, 0, 1] and got["lines"].tolist() == [1, 3, 1] and got["totals"]["not_numbers"] == 1
    # decimals at scale 2, bucketed by whole units; the measured decimal at scale 3
    got = check(gorp, data, offsets, ids, caps, [(1, 0, 1)], 100, formats=formats)
    assert got["bucket_number"].tolist() == [0, 12] and [s["sum"] for s in got["stats"]] == [250, -1000]


# ---------------------------------------------------------------------------
# end to end: the syslog workload, extracted on the device, `ts` in milliseconds, per minute
# ---------------------------------------------------------------------------
def test_syslog_lines_per_minute_end_to_end_and_from_raw_text():
    rules, meta = W.syslog_definition(4)
    gorp = Gorp.construct(rules)
    data, offsets, _ = W.syslog_lines(meta, 2000, seed=11)
    data, offsets = np.asarray(data, np.uint8), np.asarray(offsets, np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids >= 0).sum() > 1900 and (ids < 0).sum() > 5
    for k in range(4):
        gorp.set_number_format(k, "ts", "iso8601", 3)
    parts = [("rule%d" % k, "ts") for k in range(3)] + [("rule3", "ts", "pid")]
    formats = {(k, 0): ("iso8601", 3) for k in range(4)}
    origin = "2026-01-01T00:00:00Z"
    got = check(gorp, data, offsets, ids, caps, parts, 60_000, origin=origin, formats=formats, max_buckets=64)
    assert got["totals"]["n_buckets"] > 64 and got["totals"]["bucketed"] > 1800 and got["bucket_number"][0] >= 0      # (more than max_buckets: asked twice)
    # line_bucket against a search of the oracle's bucket of every line in bucket_number
    p = gorp.bucket_parts(parts)
    o = gorp._bucket_origin(p, origin)
    assert o == parse_number("iso8601", 3, origin)
    for i in np.flatnonzero(got["line_bucket"] != NONE)[::7]:
        k = int(ids[i])
        v = parse_number("iso8601", 3, bytes(data[int(offsets[i]) + caps[i, 0]:int(offsets[i]) + caps[i, 1]]))
        assert got["line_bucket"][i] == np.searchsorted(got["bucket_number"], (v - o) // 60_000) and k >= 0
    # the whole-file form: raw text in, the same buckets out
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))]
    text, counts, n_lines = gorp.text_bucket_lines(b"\n".join(lines) + b"\n", parts, 60_000, origin=origin)
    assert n_lines == len(ids) and counts[:4].tolist() == [int((ids == k).sum()) for k in range(4)]
    assert text["totals"] == got["totals"] and text["stats"] == got["stats"] and all(text[f].tobytes() == got[f].tobytes() for f in FIELDS)


# ---------------------------------------------------------------------------
# one large shape
# ---------------------------------------------------------------------------
def test_two_million_lines_against_numpy():
    gorp = trivial_handle(1)
    n = 2_000_000
    v, matched = draw(n, seed=20)
    data, offsets, ids, caps = digits_batch(v, matched)
    for origin, width, max_buckets in ((0, 60_000, 128), (123_456, 7, n)):
        number, first, lines, line_bucket = np_buckets(v, matched, origin, width)
        got = gorp.bucket_lines(data, offsets, ids, caps, P0, width, origin, max_buckets=max_buckets)
        t = got["totals"]
        assert t["n_buckets"] == len(number) and t["bucketed"] == t["lines"] == int(matched.sum()) and t["exact"]
        assert (t["first_bucket"], t["last_bucket"]) == (int(number[0]), int(number[-1]))
        for name, want in (("bucket_number", number), ("first_line", first), ("lines", lines), ("line_bucket", line_bucket)):
            assert got[name].dtype == want.dtype and np.array_equal(got[name], want), name
    assert len(number) > 500_000
