"""GPU tests of gx_top_lines / gx_text_top_lines: the lines of a finished batch ranked by a number they captured.

Expected values come from tests/top_oracle.py -- every line classed as tests/stats_oracle.py classes one, then
sorted(cands, key=(-v, line))[:N] -- and everything is compared bit for bit.  Most batches are fabricated against handles of K
identical, trivial extractions: a line is its value, its capture row (0, length), its id chosen here; the end-to-end cases take ids and
rows from gx_extract_batch."""
import ctypes as C
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from top_oracle import decode_parts, top_lines
from where_oracle import INT64_MAX, INT64_MIN, decode_terms, unpack

pytestmark = pytest.mark.gpu

PUT, GET, OTHER = 0, 1, 2  # workloads.readme3_definition: the extractions' indices; groups timestamp, verb, timeTakenInMsec, path
K3 = 3
MAXN = N.GX_TOP_MAX_LINES
KEYS_GRID = 2048 * 256     # gx_top.hip: lines of one trip of the keys pass's grid stride
SWEEP_GRID = 1024 * 1024   # ... and of a sweep's (four lines a lane)
SCAN_BLOCK = 256 * 8       # gx_scan.hpp
BY_TIME = [("GetRequest", "timeTakenInMsec")]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, by, n, largest=True, where=None, utf8=None):
    """top_lines against the restatement, every output; returns what the call returned."""
    parts = gorp.top_parts(by)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    w_index, w_values, w_units, w_off, w_totals = top_lines(data, offsets, ids, caps, decode_parts(parts), decode_terms(terms), gorp.num_extractions, n, largest)
    got = gorp.top_lines(data, offsets, ids, caps, parts, n, largest=largest, where=terms, utf8=utf8)
    index, values, data2, off2, ids2, rows2, totals = got
    assert totals == w_totals, (totals, w_totals)
    assert index.dtype == np.uint32 and values.dtype == np.int64 and data2.dtype == data.dtype and off2.dtype == offsets.dtype
    assert np.array_equal(index, w_index) and np.array_equal(values, w_values), (index[:10], w_index[:10], values[:10], w_values[:10])
    assert np.array_equal(data2, w_units) and np.array_equal(off2, w_off)
    assert np.array_equal(ids2, np.asarray(ids)[w_index.astype(np.int64)])
    if caps is not None and np.asarray(ids).ndim == 1:
        assert np.array_equal(rows2, caps[w_index.astype(np.int64)])
    else:
        assert rows2 is None
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


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def raw_call(gorp, data, offsets, ids, caps, by, n_wanted, flags=0, out=None, cap_lines=0, out_bytes_cap=0, **kw):
    """gx_top_lines itself on host arrays; out: dict of arrays by output name.  Returns (rc, totals dict)."""
    p = gorp.top_parts(by)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    out = out or {}
    ptr = lambda name: out[name].ctypes.data if name in out else None
    t = N.gx_top_totals()
    rc = N.lib().gx_top_lines(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, len(offsets) - 1, ids.ctypes.data if ids.size else None,
                              None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, n_wanted, flags, ptr("index"), ptr("values"),
                              ptr("bytes"), ptr("offsets"), ptr("ids"), ptr("caps"), cap_lines, out_bytes_cap, C.byref(t), C.byref(o))
    return rc, Gorp._top_totals(t)


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
    stats = gorp.capture_stats(data, offsets, id_col, rows, BY_TIME)[0]
    for largest in (True, False):
        for n in (1, 10, 100):
            index, values, _, _, _, _, totals = check(gorp, data, offsets, id_col, rows, BY_TIME, n, largest=largest)
            assert len(index) == n and (ids[index.astype(np.int64)] == GET).all()
            assert totals["numbers"] == totals["lines"] == stats["numbers"] == (ids == GET).sum()
            # the caller's loop, in Python: sorted(results, by timeTakenInMsec).take(N)
            took = [int(bytes(data[int(offsets[i]) + caps[i, 4]:int(offsets[i]) + caps[i, 5]])) for i in index]
            assert took == values.tolist() == sorted(took, reverse=largest)
            if n == 1:
                assert values[0] == (stats["max"] if largest else stats["min"])


# ---------------------------------------------------------------------------
# N against the number of candidates
# ---------------------------------------------------------------------------
WANTED = [0, 1, 63, 64, 65, 255, 256, 257, MAXN]


@pytest.mark.parametrize("count", [1, 2, 64, 300, MAXN + 1])
def test_n_wanted_against_the_numbers_there_are(count):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(count)
    numbers = rng.integers(-50, 50, count) if count <= 300 else rng.integers(-10 ** 6, 10 ** 6, count)   # (few values: ties at most cuts)
    data, offsets, ids, caps = numbers_batch(numbers)
    for largest in (True, False):
        for n in WANTED:
            index, _, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], n, largest=largest)
            assert len(index) == totals["n_top"] == min(n, count)                   # N > numbers delivers them all
            assert len(set(index.tolist())) == len(index)


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
def test_ties_go_to_the_earliest_lines():
    gorp = trivial_handle(2)
    # all values equal: the first N lines in order
    data, offsets, ids, caps = numbers_batch([42] * 1000)
    for largest in (True, False):
        for n in (1, 7, 64, 65, 999, 1000, 1001):
            index, values, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], n, largest=largest)
            assert index.tolist() == list(range(min(n, 1000))) and totals["ties_left"] == 1000 - min(n, 1000) and totals["last_value"] == 42
    # a threshold value held by 10 lines of which 3 are taken
    rng = np.random.default_rng(2)
    numbers = np.concatenate([np.full(10, 500), rng.integers(501, 10 ** 6, 20), rng.integers(-10 ** 6, 500, 300)])
    rng.shuffle(numbers)
    data, offsets, ids, caps = numbers_batch(numbers)
    index, values, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 23)
    assert values[-3:].tolist() == [500] * 3 and index[-3:].tolist() == np.flatnonzero(numbers == 500)[:3].tolist()
    assert totals["ties_left"] == 7 and totals["last_value"] == 500
    # "7", "007" and "+7" are the same number
    values = [b"3", b"007", b"9", b"+7", b"7", b"-7", b"0007", b"8"]
    data, offsets, ids, caps = values_batch(values)
    index, got, data2, off2, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 4)
    assert index.tolist() == [2, 7, 1, 3] and got.tolist() == [9, 8, 7, 7] and totals["ties_left"] == 2
    assert bytes(data2) == b"98007+7"
    index, got, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 4, largest=False)
    assert index.tolist() == [5, 0, 1, 3] and totals["ties_left"] == 2


# ---------------------------------------------------------------------------
# one digit of the key at a time; the edges of int64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", range(8))
def test_values_that_differ_in_one_byte_of_the_key_alone(d):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(d)
    base = 0x0102030405060708 & ~(0xFF << (8 * d))
    digits = np.concatenate([np.arange(256), rng.integers(0, 256, 244)])
    rng.shuffle(digits)
    numbers = [(base | (int(x) << (8 * d))) - 2 ** 63 for x in digits]              # the key is the value plus 2^63: byte d of the key is x
    data, offsets, ids, caps = numbers_batch(numbers)
    for largest in (True, False):
        for n in (1, 3, 100, 257, 499, 500):
            check(gorp, data, offsets, ids, caps, [(0, 0)], n, largest=largest)


def test_edge_values_in_both_directions():
    gorp = trivial_handle(1)
    values = [b"-0", b"0", b"-1", b"1", str(INT64_MIN).encode(), str(INT64_MAX).encode(), b"+0", str(INT64_MIN + 1).encode(), str(INT64_MAX - 1).encode(),
              b"-255", b"256", b"-4294967296", b"4294967295", str(INT64_MAX).encode(), str(INT64_MIN).encode(), b"-00"]
    data, offsets, ids, caps = values_batch(values)
    for n in range(len(values) + 2):
        for largest in (True, False):
            check(gorp, data, offsets, ids, caps, [(0, 0)], n, largest=largest)
    index, got, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 3)
    assert got.tolist() == [INT64_MAX, INT64_MAX, INT64_MAX - 1] and index.tolist() == [5, 13, 8]
    index, got, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 3, largest=False)
    assert got.tolist() == [INT64_MIN, INT64_MIN, INT64_MIN + 1] and index.tolist() == [4, 14, 7]
    # -0 is 0: four lines hold it, in line order
    index, got, _, _, _, _, _ = check(gorp, data, offsets, ids, caps, [(0, 0)], 10)
    assert got.tolist()[5:] == [1, 0, 0, 0, 0] and index.tolist()[6:] == [0, 1, 6, 15]


# ---------------------------------------------------------------------------
# what is no candidate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_values_that_are_no_numbers_unset_groups_and_invalid_pairs_are_never_delivered(fmt):
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
    id_col, rows = (ids, caps) if fmt == "int32" else (pack(ids, caps, np.uint16 if fmt == "u16" else np.uint8), None)
    for largest in (True, False):
        index, values, _, _, _, _, totals = check(gorp, data, offsets, id_col, rows, [(0, 0)], 100, largest=largest)
        assert (totals["numbers"], totals["unset"], totals["not_numbers"]) == (2 * 2 + 2 + 1, 6, 2 * 7 + 2)
        assert sorted(values.tolist()) == [-6, -6, 5, 5, 34, 777, 12345]
    # UTF-16 units: U+FF11 is no digit here
    wide = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31, 0x32], [0x131, 0x32], [0x2D, 0x37], [0x2D, 0xFF17], [], [0x2B, 0x39, 0x39]]
    data, offsets, ids, caps = values_batch(wide, dtype=np.uint16)
    index, values, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(0, 0)], 100)
    assert values.tolist() == [99, 12, 1, -7] and totals["not_numbers"] == 5


# ---------------------------------------------------------------------------
# terms and parts
# ---------------------------------------------------------------------------
def test_terms_and_two_parts_in_one_number_space(readme):
    gorp, data, offsets, ids, caps = readme
    matched = np.concatenate([np.ones(K3, np.uint8), np.zeros(K3 + 1, np.uint8)])
    for fmt in ("int32", "u8"):
        id_col, rows = (ids, caps) if fmt == "int32" else (gorp.extract_batch(data, offsets, compact=2)[0], None)
        # where with >=: the oracle on the filtered lines
        where = [("GetRequest", "timeTakenInMsec", ">=", 500)]
        index, values, _, _, _, _, totals = check(gorp, data, offsets, id_col, rows, BY_TIME, 50, largest=False, where=where)
        assert values.min() >= 500 and 0 < totals["lines"] < (ids == GET).sum()
        sel = gorp.select_lines_where(data, offsets, id_col, rows, where, want=matched)
        again = check(gorp, sel[1], sel[2], sel[3], sel[4] if fmt == "int32" else None, BY_TIME, 50, largest=False)
        assert np.array_equal(sel[0][again[0].astype(np.int64)], index) and np.array_equal(again[1], values) and again[6] == totals
        # two parts on two extractions; an extraction without a part never appears
        both = [("GetRequest", "timeTakenInMsec"), ("OtherRequest", "timeTakenInMsec")]
        index, values, _, _, ids2, _, totals = check(gorp, data, offsets, id_col, rows, both, 300, where=[("OtherRequest", "verb", "!=", "POST")])
        kinds = set(ids[index.astype(np.int64)].tolist())
        assert kinds == {GET, OTHER} and totals["numbers"] > (ids == GET).sum()
        index, _, _, _, _, _, totals = check(gorp, data, offsets, id_col, rows, [("OtherRequest", "timeTakenInMsec")], MAXN)
        assert len(index) == (ids == OTHER).sum() == totals["numbers"] and (ids[index.astype(np.int64)] == OTHER).all()
        # a group that holds no number: counted, never delivered
        index, _, _, _, _, _, totals = check(gorp, data, offsets, id_col, rows, [("GetRequest", "verb")], 10)
        assert len(index) == 0 and totals["not_numbers"] == (ids == GET).sum() and totals["last_value"] == 0
    # no parts, no lines wanted: legal, no lines
    index, values, data2, off2, _, _, totals = check(gorp, data, offsets, ids, caps, [], 10)
    assert len(index) == 0 and off2.tolist() == [0] and totals["lines"] == 0
    index, _, _, off2, _, _, totals = check(gorp, data, offsets, ids, caps, BY_TIME, 0)
    assert len(index) == 0 and off2.tolist() == [0] and totals["numbers"] == (ids == GET).sum()
    empty = check(gorp, data[:0], offsets[:1], ids[:0], caps[:0], BY_TIME, 10)
    assert len(empty[0]) == 0 and empty[6]["lines"] == 0


# ---------------------------------------------------------------------------
# sizes: lines, extractions
# ---------------------------------------------------------------------------
def four_byte_lines(n, K, ranked, seed, dense_tail=300, share=0.01):
    """n lines of 4 bytes; few lines of the ranked extractions except among the last `dense_tail`, where every line is one."""
    rng = np.random.default_rng(seed)
    others = np.array([k for k in {0, K // 2, K - 1, 1 % K} if k not in ranked] + [-1, -2, -1 - K], np.int32)
    ids = rng.choice(others, n)
    hit = rng.random(n) < share
    hit[max(0, n - dense_tail):] = True
    ids[hit] = rng.choice(np.array(ranked, np.int32), int(hit.sum()))
    data = rng.integers(0x30, 0x3A, 4 * n, dtype=np.uint8)
    data[rng.random(4 * n) < 0.03] = ord("-")
    offsets = (np.arange(n + 1, dtype=np.uint64) * 4).astype(np.uint32)
    caps = np.tile(np.array([0, 4], np.int32), (n, 1))
    caps[rng.random(n) < 0.1] = -1
    caps[rng.random(n) < 0.1, 0] = 2
    return data, offsets, ids.astype(np.int32), caps


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 3 * SCAN_BLOCK + 5, SWEEP_GRID + 1, KEYS_GRID + 1])
def test_line_counts_around_wave_workgroup_scan_block_and_grid_boundaries(n):
    gorp = trivial_handle(3)
    data, offsets, ids, caps = four_byte_lines(n, 3, [0, 2], seed=n)
    by = [(0, 0), (2, 0)]
    for largest, want in ((True, 100), (False, 257)):
        index, _, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, by, want, largest=largest)
        if n >= 300:
            assert len(index) == want and totals["unset"] and totals["not_numbers"]
    if n > SWEEP_GRID:
        # the line of the grid stride's second trip alone holds the largest number
        data[-4:] = np.frombuffer(b"9999", np.uint8)
        data[:-4][data[:-4] == ord("9")] = ord("8")
        caps[-1] = [0, 4]
        index, values, _, _, _, _, _ = check(gorp, data, offsets, ids, caps, by, 2)
        assert index[0] == n - 1 and values[0] == 9999 and values[1] < 9999


@pytest.mark.parametrize("K", [1, 32, 2048])
def test_extraction_counts_the_part_on_the_last(K):
    gorp = trivial_handle(K)
    data, offsets, ids, caps = four_byte_lines(6000, K, [K - 1], seed=K, share=0.3)
    index, _, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, [(K - 1, 0)], 500)
    assert len(index) == 500 and totals["unset"] > 30 and totals["not_numbers"] > 30
    # ids beyond the extractions and exceptions of the ranked one add nothing
    ids2 = ids.copy()
    ids2[ids2 < 0] = -2
    ids2[::5] = K
    check(gorp, data, offsets, ids2, caps, [(K - 1, 0)], 500, largest=False)


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
    for largest in (True, False):
        index, _, data2, _, _, _, totals = check(gorp, data, offsets, ids, caps, BY_TIME, 40, largest=largest, where=[("GetRequest", "path", "contains", "Ж")])
        assert len(index) == 40 and 0 < totals["lines"] < (ids == GET).sum() and (data2 == 0x416).any()
    for fmt in (np.uint16, np.uint8):
        check(gorp, data, offsets, pack(ids, caps, fmt), None, [("GetRequest", "verb"), ("PutRequest", "timestamp")], 30)


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
    index, _, data2, _, _, _, totals = check(gorp, data, offsets, ids, caps, BY_TIME, 200, utf8="bytes")
    assert totals["numbers"] == (ids == GET).sum() and (data2 >= 0x80).any()
    index, _, _, _, _, _, totals = check(gorp, data, offsets, ids, caps, BY_TIME, 200, largest=False, where=[("GetRequest", "path", "contains", "café")], utf8="bytes")
    assert 100 < totals["numbers"] < (ids == GET).sum() - 100
    # utf8 = 2 (offsets in units over a byte buffer) and no_sync are refused
    rc, _ = raw_call(gorp, data, offsets, ids, caps, BY_TIME, 5, utf8=2)
    assert rc == N.GX_E_ARG and "utf8" in N.last_error()
    rc, _ = raw_call(gorp, data, offsets, ids, caps, BY_TIME, 5, no_sync=1)
    assert rc == N.GX_E_ARG and "no_sync" in N.last_error()


# ---------------------------------------------------------------------------
# capacities and the size query
# ---------------------------------------------------------------------------
def test_capacities_exact_one_short_and_the_size_query(readme):
    gorp, data, offsets, ids, caps = readme
    n = 37
    w_index, w_values, w_units, w_off, w_totals = top_lines(data, offsets, ids, caps, decode_parts(gorp.top_parts(BY_TIME)), [], K3, n)
    rc, totals = raw_call(gorp, data, offsets, ids, caps, BY_TIME, n)                  # the size query
    assert rc == N.GX_OK and totals == w_totals and totals["n_top"] == n and totals["units_top"] == len(w_units)

    def fresh():
        return {"index": np.full(n + 2, 0xA5A5A5A5, np.uint32), "values": np.full(n + 2, -7, np.int64), "bytes": np.full(len(w_units) + 16, 0xA5, np.uint8),
                "offsets": np.full(n + 3, 0xA5A5A5A5, np.uint32), "ids": np.full(n + 2, 0x5A5A5A5A, np.int32), "caps": np.full((n + 2, caps.shape[1]), 0x5A5A5A5A, np.int32)}
    out = fresh()
    rc, totals = raw_call(gorp, data, offsets, ids, caps, BY_TIME, n, out=out, cap_lines=n, out_bytes_cap=len(w_units))   # exact
    assert rc == N.GX_OK and totals == w_totals
    assert np.array_equal(out["index"][:n], w_index) and np.array_equal(out["values"][:n], w_values) and np.array_equal(out["bytes"][:len(w_units)], w_units)
    assert np.array_equal(out["offsets"][:n + 1], w_off) and np.array_equal(out["ids"][:n], ids[w_index]) and np.array_equal(out["caps"][:n], caps[w_index])
    untouched = fresh()
    assert all(np.array_equal(out[k][n + (k == "offsets"):], untouched[k][n + (k == "offsets"):]) for k in out if k != "bytes")
    assert (out["bytes"][len(w_units):] == 0xA5).all()
    for short in (dict(cap_lines=n - 1, out_bytes_cap=len(w_units)), dict(cap_lines=n, out_bytes_cap=len(w_units) - 1)):   # one line short, one unit short
        out = fresh()
        rc, totals = raw_call(gorp, data, offsets, ids, caps, BY_TIME, n, out=out, **short)
        assert rc == N.GX_E_LIMIT and totals == w_totals
        assert all(np.array_equal(out[k], untouched[k]) for k in out)                  # nothing written
    # single outputs; cap_lines >= n_wanted always suffices; the byte capacity is not looked at without out_bytes
    for name in ("index", "values", "offsets", "ids", "caps"):
        out = {name: fresh()[name]}
        rc, totals = raw_call(gorp, data, offsets, ids, caps, BY_TIME, n, out=out, cap_lines=n)
        assert rc == N.GX_OK and totals == w_totals and not np.array_equal(out[name], untouched[name])
    out = {"bytes": fresh()["bytes"]}
    rc, _ = raw_call(gorp, data, offsets, ids, caps, BY_TIME, n, out=out, cap_lines=0, out_bytes_cap=len(w_units))
    assert rc == N.GX_OK and np.array_equal(out["bytes"][:len(w_units)], w_units)
    with pytest.raises(GorpError) as ei:
        gorp.top_lines(data, offsets, ids, caps, BY_TIME, MAXN + 1)
    assert ei.value.code == N.GX_E_LIMIT


# ---------------------------------------------------------------------------
# device buffers: alignment, the end of the allocation, fences, stream order, determinism
# ---------------------------------------------------------------------------
def test_device_buffers_at_every_misalignment_end_with_the_last_capture_and_fences_stay():
    import torch
    gorp = trivial_handle(4)
    rng = np.random.default_rng(21)
    n, want = 3000, 200
    values = [str(int(v)).encode() for v in rng.integers(-10 ** 6, 10 ** 12, n)]
    values[-1] = b"9223372036854775807"                                       # the last capture ends at the buffer's last byte
    data, offsets, ids, caps = values_batch(values, rng.integers(-2, 4, n))
    ids[-1] = 3
    rows8 = pack(ids, caps, np.uint8)
    by = [(3, 0), (0, 0)]
    index, vals, data2, off2, _, _, totals = check(gorp, data, offsets, ids, caps, by, want)
    assert index[0] == n - 1 and vals[0] == INT64_MAX
    d_off, d_ids, d_caps = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    F = 64   # bytes of poison on either side of every output
    for mis in range(16):
        src = torch.empty(mis + len(data), dtype=torch.uint8, device="cuda")     # sized exactly: the batch ends where the tensor ends
        src[mis:] = torch.from_numpy(data).cuda()
        d_rows = torch.empty(mis + rows8.size, dtype=torch.uint8, device="cuda")
        d_rows[mis:] = torch.from_numpy(rows8.reshape(-1)).cuda()
        sizes = {"index": want * 4, "values": want * 8, "bytes": len(data2), "offsets": (want + 1) * 4, "ids": want * 4, "caps": want * 8, "rows": want * 3}
        for compact in (0, 2):
            bufs = {k: torch.full((2 * F + sizes[k] + mis,), 0xA5, dtype=torch.uint8, device="cuda") for k in sizes}
            at = lambda k, extra=0: bufs[k].data_ptr() + F + extra
            rc, got = gorp.top_lines_device(src.data_ptr() + mis, d_off.data_ptr(), n, d_rows.data_ptr() + mis if compact else d_ids.data_ptr(),
                                            None if compact else d_caps.data_ptr(), by, want, out_index_ptr=at("index"), out_values_ptr=at("values"),
                                            out_data_ptr=at("bytes", mis), out_offsets_ptr=at("offsets"), out_ids_ptr=at("rows", mis) if compact else at("ids"),
                                            out_caps_ptr=None if compact else at("caps"), cap_lines=want, out_bytes_cap=len(data2), compact=compact,
                                            where=[(3, 0, ">=", -10 ** 7)])
            torch.cuda.synchronize()
            assert rc == N.GX_OK and got == totals
            host = {k: v.cpu().numpy() for k, v in bufs.items()}
            inner = lambda k, extra=0: host[k][F + extra:F + extra + sizes[k]]
            assert np.array_equal(inner("index").view(np.uint32), index) and np.array_equal(inner("values").view(np.int64), vals)
            assert np.array_equal(inner("bytes", mis), data2) and np.array_equal(inner("offsets").view(np.uint32), off2)
            if compact:
                assert np.array_equal(inner("rows", mis).reshape(want, 3), rows8[index.astype(np.int64)])
            else:
                assert np.array_equal(inner("ids").view(np.int32), ids[index.astype(np.int64)]) and np.array_equal(inner("caps").view(np.int32).reshape(want, 2), caps[index.astype(np.int64)])
            for k in sizes:
                used = k in (("index", "values", "bytes", "offsets", "rows") if compact else ("index", "values", "bytes", "offsets", "ids", "caps"))
                extra = mis if k in ("bytes", "rows") else 0
                assert (host[k][:F + extra] == 0xA5).all() and (host[k][F + extra + (sizes[k] if used else 0):] == 0xA5).all(), (k, mis, compact)
    # dense ids without capture rows: refused on a handle with a device too
    with pytest.raises(GorpError) as ei:
        gorp.top_lines_device(src.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), None, by, want)
    assert ei.value.code == N.GX_E_ARG


def test_the_call_follows_a_no_sync_batch_on_its_stream_and_two_runs_are_the_same_bits():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L, want = 60000, 200, 500
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.full((n, width), 0x55, dtype=torch.uint8, device="cuda")       # ids nobody wrote: outcome 2K + 1
    stream = torch.cuda.Stream()
    other = torch.cuda.Stream()
    where = [("GetRequest", "timeTakenInMsec", "<", 9000)]

    def outputs():
        return [torch.zeros(want, dtype=torch.int32, device="cuda"), torch.zeros(want, dtype=torch.int64, device="cuda"),
                torch.zeros(want * L, dtype=torch.uint8, device="cuda"), torch.zeros(want + 1, dtype=torch.int32, device="cuda"),
                torch.zeros((want, width), dtype=torch.uint8, device="cuda")]

    def run(out, s):
        return gorp.top_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, BY_TIME, want, where=where, out_index_ptr=out[0].data_ptr(),
                                     out_values_ptr=out[1].data_ptr(), out_data_ptr=out[2].data_ptr(), out_offsets_ptr=out[3].data_ptr(),
                                     out_ids_ptr=out[4].data_ptr(), cap_lines=want, out_bytes_cap=want * L, compact=2, stream=s.cuda_stream)
    a, b, c = outputs(), outputs(), outputs()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True, compact=2,
                                  line_bytes_hint=L)
        rc, got = run(a, stream)
        rc2, again = run(b, stream)
    with torch.cuda.stream(other):
        rc3, third = run(c, other)          # (another stream: it waits for the emit pass that still reads the handle's workspace)
    torch.cuda.synchronize()
    assert rc == rc2 == rc3 == N.GX_OK and got == again == third and got["n_top"] == want
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(unpack(h_rows)[0], cat.cpu().numpy().astype(np.int32))
    terms = decode_terms(gorp.where_terms(where))
    w_index, w_values, w_units, w_off, w_totals = top_lines(h_data, h_off, h_rows, None, decode_parts(gorp.top_parts(BY_TIME)), terms, K3, want)
    assert got == w_totals
    for out in (a, b, c):                                                              # two runs (three): the same bits
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), w_index) and np.array_equal(out[1].cpu().numpy(), w_values)
        assert np.array_equal(out[2].cpu().numpy()[:len(w_units)], w_units) and np.array_equal(out[3].cpu().numpy().view(np.uint32), w_off)
        assert np.array_equal(out[4].cpu().numpy(), h_rows[w_index.astype(np.int64)])


def test_the_delivered_batch_extracts_to_its_rows_and_index_composes_with_select_where(readme):
    gorp, data, offsets, ids, caps = readme
    index, values, data2, off2, ids2, rows2, totals = check(gorp, data, offsets, ids, caps, BY_TIME, 300)
    e_ids, e_caps = gorp.extract_batch(data2, off2)
    assert np.array_equal(e_ids, ids2) and np.array_equal(e_caps, rows2)
    for v in sorted(set(values.tolist())):
        sel = gorp.select_lines_where(data, offsets, ids, caps, [("GetRequest", "timeTakenInMsec", "==", int(v))], want=np.array([0, 1, 0, 0, 0, 0, 0], np.uint8))
        mine = index[values == v]
        assert np.array_equal(sel[0][:len(mine)], mine)                                # the lines that hold v, earliest first
        if v != totals["last_value"]:
            assert len(sel[0]) == len(mine)
        else:
            assert len(sel[0]) == len(mine) + totals["ties_left"]


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
def test_text_top_lines_is_split_extract_top(utf8):
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
        for largest, n in ((True, 1), (True, 150), (False, 64)):
            want = check(gorp, data, offsets, ids, caps, by, n, largest=largest, where=where, utf8="bytes" if utf8 else None)
            index, values, out, totals, counts, n_lines = gorp.text_top_lines(text, by, n, largest=largest, where=where, utf8=utf8)
            assert np.array_equal(index, want[0]) and np.array_equal(values, want[1]) and out == bytes(want[2]) and totals == want[6]
            assert n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids))
            assert out == b"".join(text[int(offsets[i]):int(offsets[i + 1])] for i in index)    # each line with its terminator as the text has it
    index, values, out, _, _, _ = gorp.text_top_lines(text, by, 2, utf8=utf8)
    assert index[0] == len(raw) and values[0] == 99999999 and out.startswith(b"[123456789]: GET 99999999ms /tail[")
    # one byte short: GX_E_LIMIT with the totals; no parts; an empty text
    room = np.zeros(len(out), np.uint8)
    rc, totals, size, _, _ = gorp.text_top_lines_device(data.ctypes.data, data.size, by, 2, out_ptr=room.ctypes.data, out_cap=len(out) - 1,
                                                         device_pointers=False, utf8=utf8)
    assert rc == N.GX_E_LIMIT and size == len(out) and totals["n_top"] == 2
    index, values, out, totals, counts, n_lines = gorp.text_top_lines(text, [], 5, utf8=utf8)
    assert len(index) == 0 and out == b"" and n_lines == len(raw) + 1 and np.array_equal(counts, gorp.count_outcomes(ids))
    index, values, out, totals, counts, n_lines = gorp.text_top_lines(b"", by, 5, utf8=utf8)
    assert len(index) == 0 and out == b"" and n_lines == 0 and counts.sum() == 0 and totals["lines"] == 0


# ---------------------------------------------------------------------------
# a batch that lives on the device, against torch's stable sort
# ---------------------------------------------------------------------------
def test_200k_lines_on_the_device_against_torch_sort():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 200000, 200
    data, offsets, cat = W.readme3_lines(n, seed=12, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    caps = torch.empty((n, 2 * gorp.max_groups), dtype=torch.int32, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
    assert torch.equal(ids, cat.to(torch.int32))
    pow10 = torch.tensor([1, 10, 100, 1000], dtype=torch.int64, device="cuda")
    sel = ids == GET
    lines = torch.nonzero(sel)[:, 0]
    b, e = caps[sel, 4].to(torch.int64), caps[sel, 5].to(torch.int64)
    nd = e - b
    assert int(nd.min()) >= 1 and int(nd.max()) <= 4
    j = torch.arange(4, device="cuda")[None, :]
    digit = data.view(n, L)[sel].gather(1, (b[:, None] + j).clamp(max=L - 1)).to(torch.int64) - 48
    v = (digit * pow10[(nd[:, None] - 1 - j).clamp(min=0)] * (j < nd[:, None])).sum(1)
    for largest in (True, False):
        order = torch.sort(v, stable=True, descending=largest)[1]
        for want in (10, MAXN):
            index = torch.zeros(want, dtype=torch.int32, device="cuda")
            values = torch.zeros(want, dtype=torch.int64, device="cuda")
            out = torch.zeros(want * L, dtype=torch.uint8, device="cuda")
            rc, totals = gorp.top_lines_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), BY_TIME, want, largest=largest,
                                               out_index_ptr=index.data_ptr(), out_values_ptr=values.data_ptr(), out_data_ptr=out.data_ptr(), cap_lines=want,
                                               out_bytes_cap=want * L)
            torch.cuda.synchronize()
            assert rc == N.GX_OK and totals["n_top"] == want and totals["numbers"] == int(sel.sum()) and totals["units_top"] == want * L
            assert torch.equal(index.to(torch.int64), lines[order[:want]]) and torch.equal(values, v[order[:want]])
            assert torch.equal(out.view(want, L), data.view(n, L)[lines[order[:want]]])
            assert totals["last_value"] == int(values[-1]) and totals["ties_left"] == int((v == values[-1]).sum() - (values == values[-1]).sum())


# ---------------------------------------------------------------------------
# the whole-file call from host buffers and from device pointers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_text_form_from_host_buffers_and_device_pointers(n):
    from twin_buffers import twins
    gorp = Gorp.construct(W.readme3_definition())
    lines = ["[%d]: %s %dms /p/%d" % (i, ("GET", "PUT", "POST")[i % 3], 10 * i, i % 7) for i in range(n)]
    if n > 9:
        lines[5], lines[9] = "", "nothing here"
    text = np.frombuffer("".join(l + "\n" for l in lines).encode(), np.uint8)
    text16 = np.zeros((text.size + 15) // 16 * 16 + 16, np.uint8)       # (a device text is 16-byte aligned: torch's allocations are)
    text16[:text.size] = text
    gets = [i for i in range(n) if i % 3 == 0 and i != 9][::-1][:4]     # the four slowest GET lines, slowest first

    def size_query(b, device_pointers):
        rc, totals, size, counts, n_lines = gorp.text_top_lines_device(b.put(text16), text.size, BY_TIME, 4, device_pointers=device_pointers)
        return rc, totals, size, counts.tolist(), n_lines
    (rc, t, size, counts, n_lines), _ = twins(size_query)
    assert rc == N.GX_OK and n_lines == n and sum(counts) == n and t["n_top"] == len(gets) and size == sum(len(lines[i]) + 1 for i in gets)

    def call(b, device_pointers):
        rc, totals, out_size, c, nl = gorp.text_top_lines_device(b.put(text16), text.size, BY_TIME, 4, out_index_ptr=b.room("index", 4 * 4),
                                                                 out_values_ptr=b.room("values", 4 * 8), out_ptr=b.room("out", size), out_cap=size,
                                                                 device_pointers=device_pointers)
        return rc, totals, out_size, c.tolist(), nl
    (rc, totals, out_size, counts2, _), rooms = twins(call)
    assert rc == N.GX_OK and totals == t and out_size == size and counts2 == counts
    assert np.frombuffer(rooms["index"], np.uint32)[:len(gets)].tolist() == gets
    assert np.frombuffer(rooms["values"], np.int64)[:len(gets)].tolist() == [10 * i for i in gets]
    assert rooms["out"][:size] == "".join(lines[i] + "\n" for i in gets).encode()
