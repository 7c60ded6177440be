"""GPU tests of gx_capture_quantiles / gx_text_capture_quantiles: nearest-rank percentiles of a number the lines of a finished batch
captured.

Expected values come from tests/quantile_oracle.py -- every line classed as tests/top_oracle.py classes one, then
sorted(values)[rank - 1] and the counts below and equal -- and everything is compared bit for bit.  Most batches are fabricated against
handles of K identical, trivial extractions: a line is its value, its capture row (0, length), its id chosen here; the end-to-end cases
take ids and rows from gx_extract_batch."""
import ctypes as C
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from quantile_oracle import ASKS, SIXTEENTHS, capture_quantiles, groups_before_digits, parting_values, quantiles_of, rule_cases
from top_oracle import decode_parts
from where_oracle import INT64_MAX, INT64_MIN, decode_terms, unpack

pytestmark = pytest.mark.gpu

PUT, GET, OTHER = 0, 1, 2  # workloads.readme3_definition: the extractions' indices; groups timestamp, verb, timeTakenInMsec, path
K3 = 3
KEYS_GRID = 2048 * 256     # gx_top.hip: lines of one trip of the keys pass's grid stride
SWEEP_TRIP = 256 * 4       # gx_quantile.hip: keys of one trip of a sweep's workgroup (a wave's: 256) ...
SWEEP_GRID = 512 * SWEEP_TRIP   # ... and of the whole grid
SCAN_BLOCK = 256 * 8       # gx_scan.hpp
BY_TIME = [("GetRequest", "timeTakenInMsec")]
P50_95_99 = [(50, 100), (95, 100), (99, 100)]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, by, asks, where=None, utf8=None):
    """capture_quantiles against the restatement; returns what the call returned."""
    parts = gorp.top_parts(by)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = capture_quantiles(data, offsets, ids, caps, decode_parts(parts), decode_terms(terms), gorp.num_extractions, asks)
    got = gorp.capture_quantiles(data, offsets, ids, caps, parts, asks, where=terms, utf8=utf8)
    assert got[1] == want[1], (got[1], want[1])
    assert got[0] == want[0], (got[0], want[0])
    assert all(type(v) is int for r in got[0] for v in r.values() if v is not None)
    if want[1]["numbers"]:
        assert all(r["below"] < r["rank"] <= r["below"] + r["equal"] for r in got[0])
    return got


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


def values_batch(values, ids=None, dtype=np.uint8):
    """a line is its value: caps (0, length)"""
    data, offsets = csr(values, dtype=dtype)
    caps = np.array([[0, len(v)] for v in values], np.int32).reshape(len(values), 2)
    return data, offsets, np.zeros(len(values), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def numbers_batch(numbers, ids=None):
    return values_batch([str(int(v)).encode() for v in numbers], ids)


def fixed_batch(values, ids=None):
    """Many lines, made with numpy: a line is a sign and seven digits, |value| < 10^7 (a '+' and leading zeros still make a number)."""
    v = np.asarray(values, np.int64)
    assert (np.abs(v) < 10 ** 7).all()
    data = np.empty((len(v), 8), np.uint8)
    data[:, 0] = np.where(v < 0, ord("-"), ord("+"))
    data[:, 1:] = (np.abs(v)[:, None] // 10 ** np.arange(6, -1, -1)) % 10 + ord("0")
    offsets = (np.arange(len(v) + 1, dtype=np.uint64) * 8).astype(np.uint32)
    caps = np.tile(np.array([0, 8], np.int32), (len(v), 1))
    return data.reshape(-1), offsets, np.zeros(len(v), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def raw_call(gorp, data, offsets, ids, caps, by, asks, **kw):
    """gx_capture_quantiles itself on host arrays.  Returns (rc, the out rows as tuples, the totals as a tuple)."""
    p = gorp.top_parts(by)
    q, n_q = Gorp.quantile_asks(asks)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    out = (N.gx_quantile_out * 16)()
    t = N.gx_quantile_totals()
    rc = N.lib().gx_capture_quantiles(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, len(offsets) - 1, ids.ctypes.data if ids.size else None,
                                      None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, q, n_q, out, C.byref(t), C.byref(o))
    return rc, [(r.value, r.rank, r.below, r.equal) for r in out], (t.lines, t.numbers, t.unset, t.not_numbers)


# ---------------------------------------------------------------------------
# the README definition, extracted for real: row formats, offset widths, the neighbours
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def readme():
    gorp = Gorp.construct(W.readme3_definition())
    n = 12000
    t_data, _, cat = W.readme3_lines(n, seed=5)
    data = t_data.numpy().copy()
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(ids, cat.numpy().astype(np.int32))
    assert (ids == GET).sum() > 4200 and (ids == PUT).sum() > 500 and (ids == OTHER).sum() > 50 and (ids == -1).sum() > 10
    took = np.array([int(bytes(data[int(offsets[i]) + caps[i, 4]:int(offsets[i]) + caps[i, 5]])) for i in np.flatnonzero(ids == GET)], np.int64)
    return gorp, data, offsets, ids, caps, took


@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_readme_definition_in_every_row_format_and_offset_width(readme, fmt, offsets_dtype):
    gorp, data, offsets, ids, caps, took = readme
    offsets = offsets.astype(offsets_dtype)
    if fmt == "int32":
        id_col, rows = ids, caps
    else:
        id_col, rows = gorp.extract_batch(data, offsets, compact=1 if fmt == "u16" else 2)[0], None
        assert np.array_equal(id_col, pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8))
    results, totals = check(gorp, data, offsets, id_col, rows, BY_TIME, ASKS)
    assert totals["numbers"] == totals["lines"] == len(took)
    # the caller's loop, in Python: sorted(results' timeTakenInMsec)[ceil(q * n) - 1]
    assert results == quantiles_of(took, ASKS)
    spelled = gorp.capture_quantiles(data, offsets, id_col, rows, BY_TIME, [0.5, "0.95", 0.99])[0]
    assert spelled == quantiles_of(took, P50_95_99)
    assert spelled[0]["value"] == int(np.quantile(took, 0.5, method="inverted_cdf")) and spelled[2]["value"] == int(np.quantile(took, 0.99, method="inverted_cdf"))


def test_the_ends_are_capture_stats_min_and_max_and_a_rank_is_top_lines_last_value(readme):
    gorp, data, offsets, ids, caps, took = readme
    stats = gorp.capture_stats(data, offsets, ids, caps, BY_TIME)[0]
    (lo, hi), totals = check(gorp, data, offsets, ids, caps, BY_TIME, [(0, 7), (7, 7)])
    assert lo["value"] == stats["min"] and hi["value"] == stats["max"] and totals["numbers"] == stats["numbers"]
    assert lo["rank"] == 1 and lo["below"] == 0 and hi["rank"] == totals["numbers"] and hi["below"] + hi["equal"] == totals["numbers"]
    numbers = totals["numbers"]
    assert numbers > 4096
    for r in (1, 2, 100, 1000, 4096):
        (got,), _ = check(gorp, data, offsets, ids, caps, BY_TIME, [(r, numbers)])
        values = gorp.top_lines(data, offsets, ids, caps, BY_TIME, r, largest=False)[1]
        assert got["rank"] == r and len(values) == r and got["value"] == values[-1]


# ---------------------------------------------------------------------------
# population sizes around every boundary a pass has
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, SWEEP_TRIP - 1, SWEEP_TRIP, SWEEP_TRIP + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_population_sizes_around_wave_trip_and_scan_block_boundaries(count):
    gorp = trivial_handle(2)
    rng = np.random.default_rng(count)
    numbers = rng.integers(-50, 50, count) if count % 2 else rng.integers(-10 ** 12, 10 ** 12, count)   # (few values: ties at every rank; or many)
    values = [str(int(v)).encode() for v in numbers]
    ids = [0] * count
    for at, (v, i) in ((0, (b"5", 1)), (count // 2 + 1, (b"x", 0)), (count + 2, (b"6", -1))):   # no part, no number, no extraction
        values.insert(at, v)
        ids.insert(at, i)
    data, offsets, ids, caps = values_batch(values, ids)
    caps[len(values) // 3] = -1                                   # (an unset pair: a number or not, it is none now)
    results, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], ASKS)
    assert count - 1 <= totals["numbers"] <= count and totals["lines"] == count + 1
    # all lines numbers: the population is the batch
    data, offsets, ids, caps = numbers_batch(numbers)
    results, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], ASKS)
    assert totals["numbers"] == count and (count == 0) == (results[0]["value"] is None)


@pytest.mark.parametrize("case", ["lines beyond the keys pass's grid", "numbers beyond the sweep's grid"])
def test_batches_beyond_a_grid(case):
    gorp = trivial_handle(2)
    rng = np.random.default_rng(len(case))
    if case.startswith("lines"):
        n = KEYS_GRID + 300
        ids = rng.choice(np.array([0, 0, 1, -1], np.int32), n)
        ids[-1] = 0
    else:
        n = SWEEP_GRID + SWEEP_TRIP + 1
        ids = np.zeros(n, np.int32)
    values = rng.integers(-9999, 10 ** 6, n)
    values[-1] = 9999999                                           # the line of the grid stride's second trip alone holds the largest number
    data, offsets, ids, caps = fixed_batch(values, ids)
    pop = values[ids == 0]
    assert len(pop) > SWEEP_GRID or n > KEYS_GRID
    results, totals = gorp.capture_quantiles(data, offsets, ids, caps, [(0, 0)], ASKS)
    assert totals == {"lines": len(pop), "numbers": len(pop), "unset": 0, "not_numbers": 0}
    assert results == quantiles_of(pop, ASKS)                     # (np.sort)
    assert results[1]["value"] == 9999999 and results[1]["equal"] == 1 and results[1]["below"] == len(pop) - 1


# ---------------------------------------------------------------------------
# candidates sparse among the lines: the compaction
# ---------------------------------------------------------------------------
def test_one_number_in_the_last_of_70000_lines_and_numbers_in_every_64th_lane():
    gorp = trivial_handle(2)
    n = 70000
    rng = np.random.default_rng(70)
    values = rng.integers(-10 ** 6, 10 ** 6, n)
    ids = np.full(n, 1, np.int32)
    ids[-1] = 0
    data, offsets, ids, caps = fixed_batch(values, ids)
    results, totals = gorp.capture_quantiles(data, offsets, ids, caps, [(0, 0)], ASKS)
    assert totals == {"lines": 1, "numbers": 1, "unset": 0, "not_numbers": 0}
    assert results == [{"value": int(values[-1]), "rank": 1, "below": 0, "equal": 1}] * 16
    for lane in (0, 63):
        ids = np.full(n, -1, np.int32)
        ids[lane::64] = 0
        results, totals = gorp.capture_quantiles(data, offsets, ids, caps, [(0, 0)], ASKS)
        assert totals["numbers"] == len(values[lane::64]) and results == quantiles_of(values[lane::64], ASKS)
    # a stretch of lines without a number as long as two scan blocks, numbers on either side
    ids = np.zeros(n, np.int32)
    ids[100:100 + 2 * SCAN_BLOCK + 7] = 1
    results, totals = gorp.capture_quantiles(data, offsets, ids, caps, [(0, 0)], ASKS)
    assert results == quantiles_of(values[ids == 0], ASKS)


# ---------------------------------------------------------------------------
# values: the cases of the rule program; prefixes that part at every digit
# ---------------------------------------------------------------------------
def test_the_cases_of_the_rule_program():
    gorp = trivial_handle(1)
    for values, asks in rule_cases():
        data, offsets, ids, caps = numbers_batch(values)
        results, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], asks)
        assert totals["numbers"] == len(values) and len(results) == len(asks)
    data, offsets, ids, caps = numbers_batch([INT64_MIN, INT64_MAX, 0])
    results, _ = check(gorp, data, offsets, ids, caps, [(0, 0)], [(0, 1), (1, 2), (1, 1)])
    assert [r["value"] for r in results] == [INT64_MIN, 0, INT64_MAX]
    # numbers == 1 with 16 quantiles; "7", "007" and "+7" are the same number
    data, offsets, ids, caps = numbers_batch([-12])
    assert check(gorp, data, offsets, ids, caps, [(0, 0)], ASKS)[0] == [{"value": -12, "rank": 1, "below": 0, "equal": 1}] * 16
    data, offsets, ids, caps = values_batch([b"3", b"007", b"9", b"+7", b"7", b"-7", b"0007", b"8"])
    (median,), _ = check(gorp, data, offsets, ids, caps, [(0, 0)], [(1, 2)])
    assert median == {"value": 7, "rank": 4, "below": 2, "equal": 4}


@pytest.mark.parametrize("repeat", [1, 300])
def test_a_population_where_every_digit_level_splits_the_16_quantiles(repeat):
    gorp = trivial_handle(1)
    parting = parting_values()
    rng = np.random.default_rng(repeat)
    values = np.array(parting * repeat, dtype=object)
    rng.shuffle(values)
    data, offsets, ids, caps = numbers_batch(values)
    results, _ = check(gorp, data, offsets, ids, caps, [(0, 0)], SIXTEENTHS)
    assert [r["value"] for r in results] == parting and all(r["equal"] == repeat for r in results)
    assert groups_before_digits([r["value"] for r in results]) == [1, 2, 3, 4, 5, 6, 7, 8]
    results, _ = check(gorp, data, offsets, ids, caps, [(0, 0)], SIXTEENTHS[::-1])      # any order
    assert [r["value"] for r in results] == parting[::-1]
    results, _ = check(gorp, data, offsets, ids, caps, [(0, 0)], [(9, 16)] * 16)        # all quantiles equal
    assert results == [results[0]] * 16 and results[0]["value"] == parting[8]


# ---------------------------------------------------------------------------
# classes, parts and terms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_unset_pairs_values_that_are_no_numbers_and_lines_of_other_outcomes(fmt):
    gorp = trivial_handle(2)
    lines, caps = [], []
    for v in (b"", b"-", b"+", b"9223372036854775808", b"-9223372036854775809", b"12a", b" 1", b"5", b"-6"):
        lines += [v, b"x" + v + b"9"]                         # the value alone, and between units that would change the number
        caps += [[0, len(v)], [1, 1 + len(v)]]
    for pair in ((-1, -1), (-1, 3), (3, 2), (0, 6), (5, 6), (6, 6), (0, 5), (5, 5), (2, 4), (0, 0)):   # the line is b"12345"
        lines.append(b"12345")
        caps.append(list(pair))
    lines.append(b"777")                                      # (the last line: "beyond the line" above stays inside the buffer)
    caps.append([0, 3])
    data, offsets = csr(lines)
    ids, caps = np.zeros(len(lines), np.int32), np.array(caps, np.int32)
    ids[3::7] = [1, -1, -2, -3, 2][:len(ids[3::7])]           # another extraction, no match, exceptions, an id beyond the extractions
    id_col, rows = (ids, caps) if fmt == "int32" else (pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8), None)
    results, totals = check(gorp, data, offsets, id_col, rows, [(0, 0)], ASKS)
    assert totals["numbers"] and totals["unset"] and totals["not_numbers"] and totals["lines"] < len(lines)
    # UTF-16 units: U+FF11 is no digit here
    wide = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31, 0x32], [0x131, 0x32], [0x2D, 0x37], [0x2D, 0xFF17], [], [0x2B, 0x39, 0x39]]
    data, offsets, ids, caps = values_batch(wide, dtype=np.uint16)
    results, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], [(0, 1), (1, 2), (1, 1)])
    assert [r["value"] for r in results] == [-7, 1, 99] and totals["not_numbers"] == 5


@pytest.mark.parametrize("K", [2, 64])
def test_parts_share_one_number_space(K):
    gorp = trivial_handle(K)
    rng = np.random.default_rng(K)
    n = 3000
    ids = rng.integers(-2, K, n).astype(np.int32)
    numbers = rng.integers(-1000, 1000, n)
    data, offsets, ids, caps = numbers_batch(numbers, ids)
    by = [(k, 0) for k in range(K)][::-1]
    results, totals = check(gorp, data, offsets, ids, caps, by, ASKS)
    assert totals["numbers"] == (ids >= 0).sum() and results == quantiles_of(numbers[ids >= 0], ASKS)
    results, totals = check(gorp, data, offsets, ids, caps, [(K - 1, 0)], ASKS)          # an extraction without a part adds nothing
    assert results == quantiles_of(numbers[ids == K - 1], ASKS)
    results, totals = check(gorp, data, offsets, ids, caps, [], ASKS)                    # no parts: legal, zeros
    assert totals == {"lines": 0, "numbers": 0, "unset": 0, "not_numbers": 0} and results == [{"value": None, "rank": 0, "below": 0, "equal": 0}] * 16
    results, totals = check(gorp, data, offsets, ids, caps, by, [])                      # no quantiles: the totals alone
    assert results == [] and totals["numbers"] == (ids >= 0).sum()
    empty = check(gorp, data[:0], offsets[:1], ids[:0], caps[:0], by, ASKS)
    assert empty[1]["lines"] == 0 and empty[0][0]["value"] is None


def test_a_term_that_removes_the_current_median(readme):
    gorp, data, offsets, ids, caps, took = readme
    (median,), totals = check(gorp, data, offsets, ids, caps, BY_TIME, [(1, 2)])
    where = [("GetRequest", "timeTakenInMsec", "!=", median["value"])]
    (after,), left = check(gorp, data, offsets, ids, caps, BY_TIME, [(1, 2)], where=where)
    assert after["value"] != median["value"] and left["numbers"] == totals["numbers"] - median["equal"]
    assert after == quantiles_of(took[took != median["value"]], [(1, 2)])[0]
    # terms on another part's extraction; a group that holds no number
    both = [("GetRequest", "timeTakenInMsec"), ("OtherRequest", "timeTakenInMsec")]
    results, totals = check(gorp, data, offsets, ids, caps, both, P50_95_99, where=[("OtherRequest", "verb", "!=", "POST"), ("GetRequest", "timeTakenInMsec", ">=", 500)])
    assert 0 < totals["numbers"] < (ids == GET).sum()
    results, totals = check(gorp, data, offsets, ids, caps, [("GetRequest", "verb")], P50_95_99)
    assert totals["not_numbers"] == (ids == GET).sum() and totals["numbers"] == 0 and results[0]["value"] is None


# ---------------------------------------------------------------------------
# code units: UTF-16, UTF-8 bytes
# ---------------------------------------------------------------------------
def test_utf16_units():
    gorp = Gorp.construct(W.readme3_definition())
    n = 600
    t_data, _, _ = W.readme3_lines(n, seed=8)
    data = t_data.numpy().astype(np.uint16)
    data[np.flatnonzero(data == ord("~"))[::3]] = 0x416
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    results, totals = check(gorp, data, offsets, ids, caps, BY_TIME, ASKS, where=[("GetRequest", "path", "contains", "Ж")])
    assert 0 < totals["lines"] < (ids == GET).sum()
    for fmt in (np.uint16, np.uint8):
        check(gorp, data, offsets, pack(ids, caps, fmt), None, [("GetRequest", "timeTakenInMsec"), ("PutRequest", "timestamp")], P50_95_99)


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
    results, totals = check(gorp, data, offsets, ids, caps, BY_TIME, ASKS, utf8="bytes")
    assert totals["numbers"] == (ids == GET).sum()
    results, totals = check(gorp, data, offsets, ids, caps, BY_TIME, P50_95_99, where=[("GetRequest", "path", "contains", "café")], utf8="bytes")
    assert 100 < totals["numbers"] < (ids == GET).sum() - 100
    # utf8 = 2 (offsets in units over a byte buffer) and no_sync are refused on a handle with a device too
    rc, _, _ = raw_call(gorp, data, offsets, ids, caps, BY_TIME, [(1, 2)], utf8=2)
    assert rc == N.GX_E_ARG and "utf8" in N.last_error()
    rc, _, _ = raw_call(gorp, data, offsets, ids, caps, BY_TIME, [(1, 2)], no_sync=1)
    assert rc == N.GX_E_ARG and "no_sync" in N.last_error()
    with pytest.raises(GorpError) as ei:
        gorp.capture_quantiles(data, offsets, ids, None, BY_TIME, [(1, 2)])
    assert ei.value.code == N.GX_E_ARG


# ---------------------------------------------------------------------------
# device buffers, streams, determinism, the neighbour's workspace
# ---------------------------------------------------------------------------
def test_device_pointers_equal_host_staging_on_any_stream_and_two_runs_are_the_same_bytes():
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n = 5000
    values = [str(int(v)).encode() for v in rng.integers(-10 ** 6, 10 ** 12, n)]
    values[-1] = b"9223372036854775807"                                       # the last capture ends at the buffer's last byte
    data, offsets, ids, caps = values_batch(values, rng.integers(-2, 4, n))
    ids[-1] = 3
    rows8 = pack(ids, caps, np.uint8)
    by = [(3, 0), (0, 0)]
    where = [(3, 0, ">=", -10 ** 5)]
    want = check(gorp, data, offsets, ids, caps, by, ASKS, where=where)
    assert want[0][1]["value"] == INT64_MAX
    assert check(gorp, data, offsets, rows8, None, by, ASKS, where=where) == want
    rc, rows, totals = raw_call(gorp, data, offsets, ids, caps, by, ASKS)
    rc2, rows2, totals2 = raw_call(gorp, data, offsets, ids, caps, by, ASKS)
    assert rc == rc2 == N.GX_OK and rows == rows2 and totals == totals2        # two calls: the same bytes
    d_data = torch.from_numpy(data).cuda()                                     # sized exactly: the batch ends where the tensor ends
    d_off, d_ids, d_caps, d_rows = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda(), torch.from_numpy(rows8).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for s in (None, stream.cuda_stream):
        got = gorp.capture_quantiles_device(d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), by, ASKS, where=where, stream=s)
        assert got == want
        got = gorp.capture_quantiles_device(d_data.data_ptr(), d_off.data_ptr(), n, d_rows.data_ptr(), None, by, ASKS, where=where, compact=2, stream=s)
        assert got == want
    # dense ids without capture rows: refused on a handle with a device too
    with pytest.raises(GorpError) as ei:
        gorp.capture_quantiles_device(d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), None, by, ASKS)
    assert ei.value.code == N.GX_E_ARG


def test_right_behind_a_top_lines_that_is_still_running_on_another_stream():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L, want = 60000, 200, 500
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), compact=2, line_bytes_hint=L)
    torch.cuda.synchronize()
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    out = [torch.zeros(want, dtype=torch.int32, device="cuda"), torch.zeros(want, dtype=torch.int64, device="cuda"), torch.zeros(want * L, dtype=torch.uint8, device="cuda")]
    where = [("GetRequest", "timeTakenInMsec", "<", 9000)]
    # the top-lines call leaves its emit pass running on its stream; the quantile call on the other stream has a workspace of its own
    rc, top_totals = gorp.top_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, BY_TIME, want, where=where, out_index_ptr=out[0].data_ptr(),
                                           out_values_ptr=out[1].data_ptr(), out_data_ptr=out[2].data_ptr(), cap_lines=want, out_bytes_cap=want * L, compact=2,
                                           stream=one.cuda_stream)
    results, totals = gorp.capture_quantiles_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, BY_TIME, ASKS, where=where, compact=2,
                                                    stream=two.cuda_stream)
    torch.cuda.synchronize()
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(unpack(h_rows)[0], cat.cpu().numpy().astype(np.int32))
    terms = decode_terms(gorp.where_terms(where))
    w_results, w_totals = capture_quantiles(h_data, h_off, h_rows, None, decode_parts(gorp.top_parts(BY_TIME)), terms, K3, ASKS)
    assert (results, totals) == (w_results, w_totals)
    from top_oracle import top_lines
    w_index, w_values, w_units, _, w_top = top_lines(h_data, h_off, h_rows, None, decode_parts(gorp.top_parts(BY_TIME)), terms, K3, want)
    assert rc == N.GX_OK and top_totals == w_top
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), w_index) and np.array_equal(out[1].cpu().numpy(), w_values)
    assert np.array_equal(out[2].cpu().numpy()[:len(w_units)], w_units)
    # the largest of them all is what the quantile call says
    assert w_values[0] == results[1]["value"] and totals["numbers"] == top_totals["numbers"]


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
def test_text_capture_quantiles_is_split_extract_quantiles(utf8):
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in text_lines(3000, 21, utf8)]
    text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 99999999ms /tail"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
    assert (ids < -1).sum() > 50 and (ids == -1).sum() > 100
    by = [("GetRequest", "timeTakenInMsec"), ("PutRequest", "timeTakenInMsec")]
    wheres = [None, [("GetRequest", "timeTakenInMsec", ">=", 500)], [("GetRequest", "path", "contains", "café" if utf8 else "/v1/"), ("PutRequest", "timeTakenInMsec", "<", 500)]]
    for where in wheres:
        want = check(gorp, data, offsets, ids, caps, by, ASKS, where=where, utf8="bytes" if utf8 else None)
        results, totals, counts, n_lines = gorp.text_capture_quantiles(text, by, ASKS, where=where, utf8=utf8)
        assert (results, totals) == want
        assert n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids))
    (top,), totals, _, _ = gorp.text_capture_quantiles(text, by, [1.0], utf8=utf8)
    assert top == {"value": 99999999, "rank": totals["numbers"], "below": totals["numbers"] - 1, "equal": 1}
    # device text; no parts; no quantiles; an empty text
    import torch
    d_text = torch.from_numpy(data.copy()).cuda()
    stream = torch.cuda.Stream()
    got = gorp.text_capture_quantiles_device(d_text.data_ptr(), d_text.numel(), by, ASKS, stream=stream.cuda_stream, utf8=utf8)
    host = gorp.text_capture_quantiles(text, by, ASKS, utf8=utf8)
    assert got[:2] == host[:2] and np.array_equal(got[2], host[2]) and got[3] == host[3]
    results, totals, counts, n_lines = gorp.text_capture_quantiles(text, [], ASKS, utf8=utf8)
    assert results[0]["value"] is None and totals["lines"] == 0 and n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids))
    results, totals, counts, n_lines = gorp.text_capture_quantiles(text, by, [], utf8=utf8)
    assert results == [] and totals == host[1] and n_lines == len(raw) + 1
    results, totals, counts, n_lines = gorp.text_capture_quantiles(b"", by, ASKS, utf8=utf8)
    assert results[0]["value"] is None and n_lines == 0 and counts.sum() == 0 and totals["lines"] == 0
