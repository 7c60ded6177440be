"""GPU tests of gx_lookup_lines / gx_text_lookup_lines: what the lines of a finished batch captured, looked up in a dictionary the caller
supplies.

Expected values come from tests/lookup_oracle.py -- a Python dict filled with setdefault(entry, j), group_oracle.py's line loop,
where_oracle.parse_long and Python's integers for the sums -- and everything is compared exactly.  Most batches are fabricated against
handles of K identical, trivial extractions: a line is its value, its capture row (0, length), its id chosen here; one end-to-end case
takes ids and rows from gx_extract_batch.  The large shapes have closed forms and are compared as arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, parse_number
from group_oracle import decode_parts, group_lines
from lookup_oracle import KEEP_HITS, KEEP_NOTHING, KEEP_OTHERS, MISS, NONE, csr_entries, first_slot, lookup_lines, same, tag
from stats_oracle import SUM_SEQUENCES
from twin_buffers import MARGIN, POISON, twins
from where_oracle import INT64_MAX, INT64_MIN, decode_terms, unpack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 2048 * 256 + 1      # gx_lookup.hip: one trip of the grid stride, plus one
LDS_KEYS = int(re.search(r"GROUP_LDS_KEYS = (\d+)", open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_group.hpp")).read()).group(1))
KEEPS = {None: KEEP_NOTHING, "hits": KEEP_HITS, "others": KEEP_OTHERS}

_handles = {}


def trivial_handle(K, groups=1):
    """K identical extractions `a(.*)...`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
    return _handles[K, groups]


def csr(lines, dtype=np.uint8, offsets_dtype=np.uint32, base=0):
    """lines: sequences of code units; base: offsets[0] (units in front of the first line that belong to nobody)"""
    offsets = (np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]) + base).astype(offsets_dtype)
    data = np.array([0x7E] * base + [u for ln in lines for u in ln], dtype=dtype)
    return data, offsets


def values_batch(values, ids, dtype=np.uint8, offsets_dtype=np.uint32):
    """a line is its value: caps (0, length)"""
    data, offsets = csr(values, dtype=dtype, offsets_dtype=offsets_dtype)
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


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, entries, keep=None, where=None, utf8=None, base=0, **kw):
    """lookup_lines against the restatement, every field and the kept batch; entries: sequences of code units.  Returns what the call returned."""
    p = gorp.group_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    entries = [tuple(int(u) for u in e) for e in entries]
    want = lookup_lines(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions, entries, KEEPS[keep])
    got = gorp.lookup_lines(data, offsets, ids, caps, p, csr(entries, data.dtype, offsets.dtype, base), keep=keep, where=terms, utf8=utf8, **kw)
    same(got, want)
    if keep:
        off = offsets.astype(np.int64)
        kept = want["kept"]
        assert got["offsets"].dtype == offsets.dtype and got["data"].dtype == data.dtype
        assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in kept])]).astype(np.int64).tolist()
        assert got["data"].tolist() == [int(u) for i in kept for u in data[off[i]:off[i + 1]]]
        assert np.array_equal(got["ids"], np.asarray(ids)[kept])
        assert (got["caps"] is None) == (caps is None) and (caps is None or np.array_equal(got["caps"], caps[kept]))
    else:
        assert "index" not in got
    return got


def plain(res):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}


def numbered(count, start=0):
    return [str(j).encode() for j in range(start, start + count)]


# ---------------------------------------------------------------------------
# lane, wave, workgroup and grid edges
# ---------------------------------------------------------------------------
EDGES = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("n", EDGES)
def test_lines_and_entries_at_every_edge(n):
    gorp = trivial_handle(2)
    for m in EDGES:
        # a line's value is a number below m + 3: three of them miss; every third line does not count, and line 5 has no key
        values = [str((7 * i) % (m + 3)).encode() for i in range(n)]
        data, offsets, ids, caps = values_batch(values, [(-1 if i % 3 == 2 else i % 2) for i in range(n)])
        if n > 5:
            caps[5] = [-1, -1]
        keep = [None, "hits", "others"][(n + m) % 3]
        got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], numbered(m), keep=keep)
        assert got["totals"]["entries"] == got["totals"]["distinct_entries"] == m and len(got["line_entry"]) == n
        if m == 0:
            assert got["totals"]["hits"] == 0 and got["totals"]["misses"] == got["totals"]["keyed"]


def test_one_grid_trip_of_one_unit_lines_plus_one():
    gorp = trivial_handle(1)
    n = GRID
    data = (np.arange(n) % 251).astype(np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint32)
    ids = np.zeros(n, np.int32)
    caps = np.tile(np.array([0, 1], np.int32), (n, 1))
    entries = [bytes([b]) for b in range(0, 251, 2)] + [b"", bytes([250, 250])]      # the even bytes; two entries nobody hits
    got = gorp.lookup_lines(data, offsets, ids, caps, [(0, 0)], entries, keep="others")
    hit = data % 2 == 0
    assert np.array_equal(got["line_entry"], np.where(hit, (data // 2).astype(np.uint32), np.uint32(MISS)))
    assert np.array_equal(got["entry_same"], np.arange(128)) and got["entry_lines"].tolist() == np.bincount(data[hit] // 2, minlength=126).tolist() + [0, 0]
    assert got["entry_first_line"].tolist() == list(range(0, 251, 2)) + [NONE, NONE]
    assert got["totals"] == {"entries": 128, "distinct_entries": 128, "hit_entries": 126, "lines": n, "keyed": n, "unset": 0, "hits": int(hit.sum()),
                             "misses": int(n - hit.sum()), "lines_out": int(n - hit.sum()), "units_out": int(n - hit.sum())}
    assert np.array_equal(got["index"], np.flatnonzero(~hit)) and np.array_equal(got["data"], data[~hit]) and np.array_equal(got["offsets"], np.arange(len(got["index"]) + 1))
    assert (got["ids"] == 0).all() and np.array_equal(got["caps"], caps[:len(got["index"])])


def test_one_grid_trip_of_entries_plus_one_against_300_lines():
    gorp = trivial_handle(1, groups=2)
    m = GRID
    digits = (np.arange(m)[:, None] // 10 ** np.arange(6, -1, -1)[None, :] % 10 + 48).astype(np.uint8)      # seven digits: neighbours differ in the LAST unit only
    eu, eo = digits.reshape(-1), (np.arange(m + 1, dtype=np.uint64) * 7).astype(np.uint32)
    picks = np.concatenate([np.arange(100) * 5003 % m, [m - 1, 0, m - 1], np.arange(m, m + 197)])               # 103 hits (two entries twice), 197 misses
    values = [b"%07d" % int(j) for j in picks]
    data, offsets = csr(values)
    caps = np.array([[0, 7, 3, 7]] * len(values), np.int32)
    got = gorp.lookup_lines(data, offsets, np.zeros(300, np.int32), caps, [(0, 0, 1)], (eu, eo))
    assert np.array_equal(got["line_entry"], np.where(picks < m, picks, MISS).astype(np.uint32))
    want_lines = np.bincount(picks[picks < m], minlength=m)
    assert np.array_equal(got["entry_same"], np.arange(m)) and np.array_equal(got["entry_lines"], want_lines)
    first = np.full(m, NONE, np.uint32)
    for i in range(299, -1, -1):
        if picks[i] < m:
            first[picks[i]] = i
    assert np.array_equal(got["entry_first_line"], first)
    assert got["totals"]["distinct_entries"] == m and got["totals"]["hit_entries"] == 101 and got["totals"]["hits"] == 103 and got["totals"]["misses"] == 197
    s = got["entry_stats"][m - 1]
    assert s == {"lines": 2, "numbers": 2, "unset": 0, "not_numbers": 0, "min": (m - 1) % 10000, "max": (m - 1) % 10000, "sum": 2 * ((m - 1) % 10000)}
    assert got["entry_stats"][1]["lines"] == 0 and got["entry_stats"][1]["min"] is None


# ---------------------------------------------------------------------------
# the workgroup's LDS table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [LDS_KEYS - 1, LDS_KEYS, LDS_KEYS + 1, 4 * LDS_KEYS])
def test_one_workgroups_lines_hit_as_many_entries_as_its_lds_table_holds_and_more(distinct):
    gorp = trivial_handle(1, groups=2)
    n = 256                                                    # one workgroup
    which = [(i * 37) % distinct for i in range(n)]            # (4 x LDS_KEYS = n: every line its own entry, most adds go to global memory)
    values = [b"k%d=" % w + str((-1) ** i * (i + 1) * 10 ** (i % 17)).encode() for i, w in enumerate(which)]
    data, offsets = csr(values)
    caps = np.array([[0, v.index(b"="), v.index(b"=") + 1, len(v)] for v in values], np.int32)
    entries = [b"k%d" % j for j in range(distinct + 2)]
    got = check(gorp, data, offsets, np.zeros(n, np.int32), caps, [(0, 0, 1)], entries, keep="hits")
    assert got["totals"]["hit_entries"] == min(distinct, n) and got["totals"]["hits"] == n and int(got["entry_lines"].sum()) == n


# ---------------------------------------------------------------------------
# probing
# ---------------------------------------------------------------------------
def test_weak_hash_walks_whole_chains_and_changes_nothing():
    gorp = trivial_handle(2)
    entries = numbered(200, 1000)                                # eight hashes, tag 0: every compare is of units
    # hits, misses of an entry's length that differ from one in ONE unit (tag and length are shared), a proper prefix, an extension, the empty key
    values = [entries[(i * 13) % 200] for i in range(150)] + [b"1x00", b"100x", b"x000", b"1200", b"2000", b"999", b"100", b"10000", b"1", b""] * 3
    data, offsets, ids, caps = values_batch(values, [i % 2 for i in range(len(values))])
    strong = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], entries, keep="others")
    weak = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], entries, keep="others", weak_hash=True)
    assert plain(weak) == plain(strong) and weak["totals"]["misses"] == 30 and weak["totals"]["hits"] == 150
    assert all(tag(e, weak=True) == 0 for e in entries[:8])


def chained(slots_wanted, m, count, taken=(), length=None):
    """`count` texts whose probe starts in one of slots_wanted in the table of m entries (the oracle's hash), none of them in `taken`"""
    out, j = [], 0
    while len(out) < count:
        t = b"w%d" % j
        j += 1
        if first_slot(t, m) in slots_wanted and t not in taken and (length is None or len(t) == length):
            out.append(t)
    return out


def test_chains_that_start_in_the_last_slots_wrap_to_slot_zero():
    gorp = trivial_handle(1)
    entries = chained({61, 62, 63}, 7, 7)                          # seven entries, a 64-slot table: they fill 61, 62, 63, 0, 1, 2, 3 in some order
    assert all(first_slot(e, 7) >= 61 for e in entries)
    misses = chained({61, 62, 63, 0, 1, 2, 3}, 7, 12, taken=set(entries))      # their probes start inside the chain and end at its first empty slot
    values = (entries + misses) * 3
    data, offsets, ids, caps = values_batch(values, np.zeros(len(values)))
    got = check(gorp, data, offsets, ids, caps, [(0, 0)], entries, keep="hits")
    assert got["totals"]["hits"] == 21 and got["totals"]["misses"] == 36 and got["entry_lines"].tolist() == [3] * 7
    for order in (entries[::-1], entries[3:] + entries[:3]):      # whoever claims a slot first, the same answers
        again = check(gorp, data, offsets, ids, caps, [(0, 0)], order)
        assert again["totals"]["hits"] == 21 and again["entry_lines"].tolist() == [3] * 7


def test_prefixes_extensions_and_the_empty_key():
    gorp = trivial_handle(1)
    values = [b"", b"a", b"ab", b"abc", b"abcd", b"abd", b"b", b""]
    data, offsets, ids, caps = values_batch(values, np.zeros(len(values)))
    with_empty = check(gorp, data, offsets, ids, caps, [(0, 0)], [b"abc", b"", b"ab"], keep="others")
    assert with_empty["line_entry"].tolist() == [1, MISS, 2, 0, MISS, MISS, MISS, 1]
    without = check(gorp, data, offsets, ids, caps, [(0, 0)], [b"abc", b"ab"], keep="hits")
    assert without["line_entry"].tolist() == [MISS, MISS, 1, 0, MISS, MISS, MISS, MISS]
    only_empty = check(gorp, data, offsets, ids, caps, [(0, 0)], [b""], base=5)       # (entry_offsets[0] == 5: no unit of the dictionary is ever read)
    assert only_empty["totals"]["hits"] == 2 and only_empty["entry_lines"].tolist() == [2] and only_empty["entry_first_line"].tolist() == [0]


# ---------------------------------------------------------------------------
# duplicates
# ---------------------------------------------------------------------------
def test_duplicate_entries_are_the_lowest_of_them_on_every_run():
    gorp = trivial_handle(1, groups=2)
    values = [b"%06d" % ((i * 7919) % 400) for i in range(300)] + [b"000000"] * 3
    data, offsets = csr(values)
    caps = np.array([[0, 6, 4, 6]] * len(values), np.int32)
    ids = np.zeros(len(values), np.int32)
    # entries 0 and 70 000 with the same text
    far = [b"%06d" % j for j in range(70000)] + [b"000000"]
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1)], far)
    assert got["entry_same"][70000] == 0 and got["entry_lines"][70000] == 0 and got["entry_lines"][0] == 4 and got["entry_first_line"][70000] == NONE
    assert got["totals"]["distinct_entries"] == 70000 and got["entry_stats"][70000]["lines"] == 0 and got["entry_stats"][0]["lines"] == 4
    # all 300 entries with the same text
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1)], [b"000000"] * 300, keep="hits")
    assert got["entry_same"].tolist() == [0] * 300 and got["entry_lines"].tolist() == [4] + [0] * 299 and got["totals"]["distinct_entries"] == 1
    assert got["totals"]["hit_entries"] == 1 and set(got["line_entry"].tolist()) == {0, MISS}
    # a dictionary that is another's entries twice over
    once = [b"%06d" % j for j in range(0, 400, 3)]
    single = check(gorp, data, offsets, ids, caps, [(0, 0, 1)], once)
    double = check(gorp, data, offsets, ids, caps, [(0, 0, 1)], once + once)
    k = len(once)
    assert double["entry_same"].tolist() == list(range(k)) * 2 and double["entry_lines"].tolist() == single["entry_lines"].tolist() + [0] * k
    assert np.array_equal(double["line_entry"], single["line_entry"]) and double["totals"]["distinct_entries"] == k
    assert double["entry_stats"][:k] == single["entry_stats"]
    # two runs of the same call: bit for bit the same
    assert plain(check(gorp, data, offsets, ids, caps, [(0, 0, 1)], once + once)) == plain(double)


# ---------------------------------------------------------------------------
# readers: row formats, offset widths, code units, pairs that name no value, parts, terms, numbers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
@pytest.mark.parametrize("keep", ["hits", "others"])
def test_every_row_format_and_offset_width_with_both_keeps(fmt, offsets_dtype, keep):
    gorp = trivial_handle(3, groups=2)
    rng = np.random.default_rng(5)
    pool = numbered(40)
    values = [pool[j] + b":" + str(int(v)).encode() for j, v in zip(rng.integers(0, 40, 500), rng.integers(-1000, 1000, 500))]
    data, offsets = csr(values, offsets_dtype=offsets_dtype)
    caps = np.array([[0, v.index(b":"), v.index(b":") + 1, len(v)] for v in values], np.int32)
    caps[::17, 0] = -1                                             # no key
    caps[::19, 2:] = -1                                            # no number
    ids = rng.integers(-2, 3, 500).astype(np.int32)
    id_col, rows = in_format(ids, caps, fmt)
    # several parts on one dictionary; a term that fails on some lines, which then do not count and are not kept
    got = check(gorp, data, offsets, id_col, rows, [(0, 0, 1), (1, 0), (2, 0, 1)], pool[::2] + [b"", b"40"], keep=keep, where=[(2, 1, ">=", 0)], base=3)
    assert got["totals"]["unset"] > 0 and got["totals"]["hits"] > 50 and got["totals"]["misses"] > 50 and got["offsets"].dtype == offsets_dtype
    assert got["totals"]["lines"] < (ids >= 0).sum()


def test_utf16_units_above_0xff_in_keys_and_entries():
    gorp = trivial_handle(2)
    lines = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31], [0x3100], [0xFF11], [], [0x416, 0x16], [0x16, 0x416], [0xFF11, 0x31], [0x0031, 0x0000], []]
    data, offsets = csr(lines * 2, dtype=np.uint16)
    ids = np.array([0] * len(lines) + [1] * len(lines), np.int32)
    caps = np.array([[0, len(ln)] for ln in lines * 2], np.int32)
    entries = [[0xFF11], [0x16, 0x416], [0x31], [0x11], [0x3100], [0xFF11, 0x31, 0x31]]      # (0x11 and 0x31 0x00: what a byte-wise reader would confuse)
    got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], entries, keep="others")
    assert got["entry_lines"].tolist() == [4, 2, 4, 0, 2, 0] and got["data"].dtype == np.uint16
    for fmt in ("u16", "u8"):
        id_col, _ = in_format(ids, caps, fmt)
        assert plain(check(gorp, data, offsets, id_col, None, [(0, 0), (1, 0)], entries, keep="others"))["line_entry"] == got["line_entry"].tolist()
    listed = gorp.lookup_lines(data, offsets, ids, caps, [(0, 0), (1, 0)], ["１", "\x16Ж", "1"])
    assert listed["entry_lines"].tolist() == [4, 2, 4]


def test_utf8_bytes_with_two_three_and_four_byte_characters():
    gorp = trivial_handle(1)
    words = ["café", "Ж€", "𝄞clef", "cafe", "Ж", "€", "𝄞", "café", ""]
    values = [w.encode("utf-8") for w in words] * 3
    data, offsets, ids, caps = values_batch(values, np.zeros(len(values)))
    entries = [w.encode("utf-8") for w in ("café", "𝄞clef", "Ж€", "€")]
    got = check(gorp, data, offsets, ids, caps, [(0, 0)], entries, keep="hits", utf8="bytes")
    assert got["entry_lines"].tolist() == [6, 3, 3, 3]
    listed = gorp.lookup_lines(data, offsets, ids, caps, [(0, 0)], ["café", "𝄞clef", "Ж€", "€"], utf8="bytes")
    assert np.array_equal(listed["line_entry"], got["line_entry"])


@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_pairs_that_name_no_value_are_never_dereferenced(fmt):
    import torch
    gorp = trivial_handle(2, groups=2)
    pairs = [(-1, -1), (0, 0), (-1, 3), (5, 5), (3, 2), (0, 5), (0, 6), (2, 2), (5, 6), (6, 6), (2, 4), (0, 0), (-1, -1), (100, 200), (2, 100)]   # the line is b"12345"
    lines, caps, ids = [], [], []
    for k in (0, 1):
        for b, e in pairs:
            lines.append(b"12345")
            caps.append([b, e, 1, 3])
            ids.append(k)
    data, offsets = csr(lines)
    ids, caps = np.array(ids, np.int32), np.array(caps, np.int32)
    id_col, rows = in_format(ids, caps, fmt)
    entries = [b"34", b"", b"12345", b"1234"]
    got = check(gorp, data, offsets, id_col, rows, [(0, 0, 1), (1, 0)], entries, keep="others")
    bad = np.array([not (0 <= b <= e <= 5) for b, e in pairs] * 2)
    assert got["totals"]["unset"] == bad.sum() == 2 * 9 and ((got["line_entry"] == NONE) == bad).all() and got["totals"]["misses"] == 0
    assert got["totals"]["lines_out"] == bad.sum()
    # on the device the batch ends where its allocation ends: a pair beyond the line has nothing behind it
    d_data = torch.from_numpy(data).cuda()
    d_off = torch.from_numpy(offsets.view(np.int32)).cuda()
    d_ids = torch.from_numpy(np.ascontiguousarray(id_col).reshape(-1).view(np.uint8)).cuda()
    d_caps = None if rows is None else torch.from_numpy(rows).cuda()
    eu, eo = csr(entries)
    d_eu, d_eo = torch.from_numpy(eu).cuda(), torch.from_numpy(eo.view(np.int32)).cuda()
    le = torch.full((len(lines),), 7, dtype=torch.int32, device="cuda")
    rc, totals = gorp.lookup_lines_device(d_data.data_ptr(), d_off.data_ptr(), len(lines), d_ids.data_ptr(), None if d_caps is None else d_caps.data_ptr(),
                                          [(0, 0, 1), (1, 0)], d_eu.data_ptr(), d_eo.data_ptr(), len(entries), line_entry_ptr=le.data_ptr(),
                                          compact={"int32": 0, "u16": 1, "u8": 2}[fmt])
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals == got["totals"] | {"lines_out": 0, "units_out": 0} and np.array_equal(le.cpu().numpy().view(np.uint32), got["line_entry"])


@pytest.mark.parametrize("name", ["up", "down", "mixed"])
def test_128_bit_sums_and_the_corners_of_int64_per_entry(name):
    gorp = trivial_handle(1, groups=2)
    numbers = [str(v).encode() for count, v in SUM_SEQUENCES[name] for _ in range(count)][::7]     # every seventh: the sums still leave int64
    numbers += [str(INT64_MAX).encode(), str(INT64_MIN).encode(), b"9223372036854775808", b"-9223372036854775809", b"+0", b"x"]
    rng = np.random.default_rng(3)
    rng.shuffle(numbers)
    which = rng.integers(0, 4, len(numbers))
    keys = [b"a", b"bb", b"a" * 21, b"miss"]
    lines = [keys[w] + v for w, v in zip(which, numbers)]
    data, offsets = csr(lines)
    caps = np.array([[0, len(keys[w]), len(keys[w]), len(ln)] for w, ln in zip(which, lines)], np.int32)
    got = check(gorp, data, offsets, np.zeros(len(lines), np.int32), caps, [(0, 0, 1)], [b"bb", b"a" * 21, b"none", b"a"])
    assert got["entry_stats"][2] == {"lines": 0, "numbers": 0, "unset": 0, "not_numbers": 0, "min": None, "max": None, "sum": 0}
    assert any(not INT64_MIN <= s["sum"] <= INT64_MAX for s in got["entry_stats"])


def test_a_number_format_of_the_handles_is_honoured():
    pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(2)]
    formatted = Gorp.construct([FlattenedExtraction("r0", pieces)])        # (a handle of its own: the format stays with it)
    formatted.set_number_format(0, 1, "decimal", 2)
    texts = [b"1.5", b"2.25", b"-0.01", b"12", b"1.5", b"abc", b"", b"7.00", b"99999.99"]
    keys = [b"k1", b"k1", b"k2", b"k1", b"k3", b"k2", b"k2", b"k2", b"k1"]
    # the twin batch: every value replaced by str(number) as the host parser reads it under the format, `x` where it is no number
    numbers = [parse_number("decimal", 2, t) for t in texts]
    assert numbers[:4] == [150, 225, -1, 1200] and numbers[5] is None
    twin_texts = [b"x" if v is None else b"%d" % v for v in numbers]
    ids = np.zeros(len(texts), np.int32)
    results = []
    for gorp, vals in ((formatted, texts), (trivial_handle(1, groups=2), twin_texts)):
        lines = [k + b"=" + v for k, v in zip(keys, vals)]
        data, offsets = csr(lines)
        caps = np.array([[0, 2, 3, len(ln)] for ln in lines], np.int32)
        if gorp is formatted:
            results.append(gorp.lookup_lines(data, offsets, ids, caps, [(0, 0, 1)], [b"k2", b"k1"], where=[(0, 1, "<", 5000000)]))
        else:
            results.append(check(gorp, data, offsets, ids, caps, [(0, 0, 1)], [b"k2", b"k1"], where=[(0, 1, "<", 5000000)]))
    assert plain(results[0]) == plain(results[1])
    assert results[0]["entry_stats"][1]["sum"] == 150 + 225 + 1200 and results[0]["entry_stats"][0]["min"] == -1 and results[0]["totals"]["lines"] == 6


# ---------------------------------------------------------------------------
# keep: capacities, the size query, nothing kept, the kept batch as an ordinary batch
# ---------------------------------------------------------------------------
def raw_call(gorp, data, offsets, ids, caps, parts, entries, keep, cap_lines, bytes_cap, want=("line_entry", "entry_same", "entry_lines", "entry_first_line", "index",
             "bytes", "offsets", "ids", "caps"), poison=0xAB):
    """gx_lookup_lines itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.group_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    n, m = len(offsets) - 1, len(entries)
    eu, eo = csr(entries)
    sizes = {"line_entry": n * 4, "entry_same": m * 4, "entry_lines": m * 8, "entry_first_line": m * 4, "index": n * 4, "bytes": len(data), "offsets": (n + 1) * 4, "ids": n * 4,
             "caps": caps.size * 4}
    arrays = {k: np.full(v + 8, poison, np.uint8) for k, v in sizes.items()}
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_lookup_out(ptr("line_entry"), ptr("entry_same"), ptr("entry_lines"), ptr("entry_first_line"), None, ptr("index"), ptr("bytes"), ptr("offsets"), ptr("ids"),
                          ptr("caps"), cap_lines, bytes_cap)
    totals = N.gx_lookup_totals()
    rc = N.lib().gx_lookup_lines(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data, p.array, p.n, None, 0, eu.ctypes.data, eo.ctypes.data,
                                 m, keep, 0, C.byref(out), C.byref(totals), C.byref(o))
    return rc, Gorp._lookup_totals(totals), arrays


def test_capacities_one_short_the_size_query_and_nothing_kept():
    gorp = trivial_handle(1)
    values = numbered(100)
    data, offsets, ids, caps = values_batch(values, np.zeros(100))
    entries = numbered(30, 10)
    full = check(gorp, data, offsets, ids, caps, [(0, 0)], entries, keep="hits")
    t = full["totals"]
    assert t["lines_out"] == 30 and t["units_out"] == 60
    for cap_lines, bytes_cap, word in ((29, 60, "cap_lines"), (30, 59, "capacity")):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, KEEP_HITS, cap_lines, bytes_cap)
        assert rc == N.GX_E_LIMIT and word in N.last_error() and totals == t
        assert all((a == 0xAB).all() for a in arrays.values())                  # every output still poison, the per-entry ones too
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, KEEP_HITS, 30, 60)
    assert rc == N.GX_OK and totals == t and arrays["index"][:120].view(np.uint32).tolist() == list(range(10, 40)) and (arrays["index"][120:] == 0xAB).all()
    assert arrays["bytes"][:60].tobytes() == b"".join(values[10:40]) and (arrays["bytes"][60:] == 0xAB).all() and (arrays["offsets"][31 * 4:] == 0xAB).all()
    # the size query: no output at all
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, KEEP_HITS, 0, 0, want=())
    assert rc == N.GX_OK and totals == t and all((a == 0xAB).all() for a in arrays.values())
    # only bytes wanted: cap_lines is not looked at
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, KEEP_HITS, 0, 60, want=("bytes",))
    assert rc == N.GX_OK and arrays["bytes"][:60].tobytes() == b"".join(values[10:40])
    # nothing kept: the offsets' one entry
    none = check(gorp, data, offsets, ids, caps, [(0, 0)], numbered(5, 500), keep="hits")
    assert none["totals"]["lines_out"] == 0 and none["offsets"].tolist() == [0] and len(none["index"]) == 0
    # batch outputs with GX_LOOKUP_KEEP_NOTHING, and keep = 3
    rc, _, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, KEEP_NOTHING, 100, 1000)
    assert rc == N.GX_E_ARG and all((a == 0xAB).all() for a in arrays.values())
    rc, _, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0)], entries, 3, 100, 1000)
    assert rc == N.GX_E_ARG and "keep" in N.last_error()


def test_the_kept_batch_is_an_ordinary_batch_for_group_lines():
    gorp = trivial_handle(2, groups=2)
    rng = np.random.default_rng(8)
    values = [b"u%d %d" % (rng.integers(0, 60), rng.integers(0, 1000)) for _ in range(700)]
    data, offsets = csr(values)
    caps = np.array([[0, v.index(b" "), v.index(b" ") + 1, len(v)] for v in values], np.int32)
    ids = rng.integers(-1, 2, 700).astype(np.int32)
    known = [b"u%d" % j for j in range(0, 60, 2)]
    parts = [(0, 0, 1), (1, 0, 1)]
    others = check(gorp, data, offsets, ids, caps, parts, known, keep="others")
    # the new keys of this batch: group the others (insert-on-miss is this call and gx_group_lines)
    grouped = gorp.group_lines(others["data"], others["offsets"], others["ids"], others["caps"], parts)
    assert sorted(grouped["keys"]) == sorted(set(v.split()[0] for v, i in zip(values, ids) if i >= 0) - set(known))
    whole = gorp.group_lines(data, offsets, ids, caps, parts)
    by_key = dict(zip(whole["keys"], whole["lines"].tolist()))
    assert grouped["lines"].tolist() == [by_key[k] for k in grouped["keys"]]
    for fmt in ("u16", "u8"):
        rows, _ = in_format(ids, caps, fmt)
        o2 = check(gorp, data, offsets, rows, None, parts, known, keep="others")
        g2 = gorp.group_lines(o2["data"], o2["offsets"], o2["ids"], None, parts)
        assert g2["keys"] == grouped["keys"] and g2["lines"].tolist() == grouped["lines"].tolist() and g2["stats"] == grouped["stats"]


# ---------------------------------------------------------------------------
# twins: host buffers and device pointers leave the same bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [None, "hits", "others"])
def test_host_buffers_and_device_pointers_leave_the_same_bytes(keep):
    gorp = trivial_handle(2, groups=2)
    rng = np.random.default_rng(13)
    values = [b"h%d %d" % (rng.integers(0, 50), rng.integers(-50, 50)) for _ in range(900)]
    data, offsets = csr(values)
    caps = np.array([[0, v.index(b" "), v.index(b" ") + 1, len(v)] for v in values], np.int32)
    caps[::23, 0] = -1
    ids = rng.integers(-2, 2, 900).astype(np.int32)
    entries = [b"h%d" % j for j in range(0, 80, 3)] + [b"h3", b""]
    eu, eo = csr(entries, base=4)
    n, m = 900, len(entries)
    want = lookup_lines(data, offsets, ids, caps, [(0, 0, 1), (1, 0, -1)], [], 2, [tuple(e) for e in entries], KEEPS[keep])

    def call(b, on_device):
        rooms = dict(line_entry_ptr=b.room("line_entry", n * 4), entry_same_ptr=b.room("entry_same", m * 4), entry_lines_ptr=b.room("entry_lines", m * 8),
                     entry_first_line_ptr=b.room("entry_first_line", m * 4), entry_stats_ptr=b.room("entry_stats", m * 64))
        if keep:
            k, u = want["totals"]["lines_out"], want["totals"]["units_out"]
            rooms.update(out_index_ptr=b.room("index", k * 4), out_data_ptr=b.room("data", u), out_offsets_ptr=b.room("offsets", (k + 1) * 4),
                         out_ids_ptr=b.room("ids", k * 4), out_caps_ptr=b.room("caps", k * 16), cap_lines=k, out_bytes_cap=u)
        rc, totals = gorp.lookup_lines_device(b.put(data), b.put(offsets), n, b.put(ids), b.put(caps), [(0, 0, 1), (1, 0)], b.put(eu), b.put(eo), m, keep=keep,
                                              device_pointers=on_device, **rooms)
        return rc, totals

    (rc, totals), rooms = twins(call)
    assert rc == N.GX_OK and totals == want["totals"]
    assert np.frombuffer(rooms["line_entry"][:n * 4], np.uint32).tolist() == want["line_entry"] and rooms["line_entry"][n * 4:] == bytes([POISON]) * MARGIN
    assert np.frombuffer(rooms["entry_same"][:m * 4], np.uint32).tolist() == want["entry_same"]
    assert np.frombuffer(rooms["entry_lines"][:m * 8], np.uint64).tolist() == want["entry_lines"]
    if keep:
        assert np.frombuffer(rooms["index"][:-MARGIN], np.uint32).tolist() == want["kept"] and rooms["data"][-MARGIN:] == bytes([POISON]) * MARGIN


# ---------------------------------------------------------------------------
# the round trip that motivates the call: the keys of batch A, on the device, as batch B's dictionary
# ---------------------------------------------------------------------------
def test_keys_left_on_the_device_by_group_lines_are_the_next_batchs_dictionary():
    import torch
    gorp = trivial_handle(1, groups=2)
    rng = np.random.default_rng(17)

    def batch(lo, hi, n):
        values = [b"c%d %d" % (rng.integers(lo, hi), rng.integers(0, 10 ** 6)) for _ in range(n)]
        data, offsets = csr(values)
        caps = np.array([[0, v.index(b" "), v.index(b" ") + 1, len(v)] for v in values], np.int32)
        return data, offsets, np.zeros(n, np.int32), caps

    parts = [(0, 0, 1)]
    A, B = batch(0, 200, 1500), batch(100, 300, 1500)              # B shares half its keys with A
    dev = lambda t: [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in t]
    dA, dB = dev(A), dev(B)
    host_A = gorp.group_lines(*A, parts, keys="csr")
    k, u = host_A["totals"]["n_keys"], host_A["totals"]["key_units"]
    units = torch.zeros(u, dtype=torch.uint8, device="cuda")
    koff = torch.zeros(k + 1, dtype=torch.int32, device="cuda")
    key_lines = torch.zeros(k, dtype=torch.int64, device="cuda")
    key_stats = torch.zeros((k, 8), dtype=torch.int64, device="cuda")
    line_key = torch.zeros(1500, dtype=torch.int32, device="cuda")
    rc, _ = gorp.group_lines_device(dA[0].data_ptr(), dA[1].data_ptr(), 1500, dA[2].data_ptr(), dA[3].data_ptr(), parts, key_units_ptr=units.data_ptr(), key_units_cap=u,
                                    key_offsets_ptr=koff.data_ptr(), key_lines_ptr=key_lines.data_ptr(), key_stats_ptr=key_stats.data_ptr(),
                                    line_key_ptr=line_key.data_ptr(), max_keys=k)
    assert rc == N.GX_OK
    # A against its own keys: line_entry is line_key, entry_lines key_lines, entry_stats key_stats; nothing misses and no entry is a duplicate
    line_entry = torch.zeros(1500, dtype=torch.int32, device="cuda")
    same_ = torch.zeros(k, dtype=torch.int32, device="cuda")
    e_lines = torch.zeros(k, dtype=torch.int64, device="cuda")
    e_stats = torch.zeros((k, 8), dtype=torch.int64, device="cuda")
    rc, totals = gorp.lookup_lines_device(dA[0].data_ptr(), dA[1].data_ptr(), 1500, dA[2].data_ptr(), dA[3].data_ptr(), parts, units.data_ptr(), koff.data_ptr(), k,
                                          line_entry_ptr=line_entry.data_ptr(), entry_same_ptr=same_.data_ptr(), entry_lines_ptr=e_lines.data_ptr(),
                                          entry_stats_ptr=e_stats.data_ptr())
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["misses"] == 0 and totals["hits"] == 1500 and totals["distinct_entries"] == totals["hit_entries"] == k
    assert torch.equal(line_entry, line_key) and torch.equal(e_lines, key_lines) and torch.equal(e_stats, key_stats) and same_.tolist() == list(range(k))
    # B against A's keys, still on the device, matches the oracle on host copies
    entries = csr_entries(host_A["key_units"], host_A["key_offsets"])
    want = lookup_lines(*B, [(0, 0, 1)], [], 1, entries, KEEP_OTHERS)
    kept, ku = want["totals"]["lines_out"], want["totals"]["units_out"]
    o_data = torch.zeros(ku, dtype=torch.uint8, device="cuda")
    o_off = torch.zeros(kept + 1, dtype=torch.int32, device="cuda")
    o_ids = torch.zeros(kept, dtype=torch.int32, device="cuda")
    o_caps = torch.zeros((kept, 4), dtype=torch.int32, device="cuda")
    rc, totals = gorp.lookup_lines_device(dB[0].data_ptr(), dB[1].data_ptr(), 1500, dB[2].data_ptr(), dB[3].data_ptr(), parts, units.data_ptr(), koff.data_ptr(), k,
                                          keep="others", line_entry_ptr=line_entry.data_ptr(), entry_lines_ptr=e_lines.data_ptr(), out_data_ptr=o_data.data_ptr(),
                                          out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(), out_caps_ptr=o_caps.data_ptr(), cap_lines=kept, out_bytes_cap=ku)
    assert rc == N.GX_OK and totals == want["totals"] and 0 < totals["misses"] < 1500
    # KEEP_OTHERS followed by group_lines on the kept batch, left on the device: B's new keys, in order of appearance
    rc, g_totals = gorp.group_lines_device(o_data.data_ptr(), o_off.data_ptr(), kept, o_ids.data_ptr(), o_caps.data_ptr(), parts, max_keys=kept)
    torch.cuda.synchronize()
    assert line_entry.cpu().numpy().view(np.uint32).tolist() == want["line_entry"] and e_lines.tolist() == want["entry_lines"]
    whole_B = group_lines(*B, [(0, 0, 1)], [], 1)
    new_keys = [key for key in whole_B["keys"] if key not in set(entries)]
    assert rc == N.GX_OK and g_totals["n_keys"] == len(new_keys) == len(set(whole_B["keys"]) - set(entries)) and g_totals["lines"] == kept


# ---------------------------------------------------------------------------
# device offsets that go backwards; the whole-file form; the README definition end to end
# ---------------------------------------------------------------------------
def test_offsets_on_the_device_that_go_backwards_are_refused_by_the_pass_that_reads_them():
    import torch
    gorp = trivial_handle(1)
    data, offsets, ids, caps = values_batch(numbered(50), np.zeros(50))
    eu, eo = csr(numbered(20))
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    d_data, d_ids, d_caps, d_eu = t(data), t(ids), t(caps), t(eu)
    le = torch.full((50,), 7, dtype=torch.int32, device="cuda")
    for bad_lines, bad_entries in ((True, False), (False, True)):
        off, e_off = offsets.copy(), eo.copy()
        if bad_lines:
            off[25] = off[24] - 1                                  # (line 24 is one unit short of nothing: its length wraps to 4 G)
        if bad_entries:
            e_off[10] = e_off[9] - 1
        d_off, d_eo = t(off), t(e_off)
        with pytest.raises(GorpError) as ei:
            gorp.lookup_lines_device(d_data.data_ptr(), d_off.data_ptr(), 50, d_ids.data_ptr(), d_caps.data_ptr(), [(0, 0)], d_eu.data_ptr(), d_eo.data_ptr(), 20,
                                     line_entry_ptr=le.data_ptr())
        torch.cuda.synchronize()
        assert ei.value.code == N.GX_E_LIMIT and (le == 7).all()
        # the same offsets in host memory are found on the host
        with pytest.raises(GorpError) as ei:
            gorp.lookup_lines(data, off, ids, caps, [(0, 0)], (eu, e_off))
        assert ei.value.code == N.GX_E_LIMIT


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


VERB_PARTS = [("PutRequest", "verb", "timeTakenInMsec"), ("GetRequest", "verb", "timeTakenInMsec"), ("OtherRequest", "verb", "timeTakenInMsec")]


def test_readme_definition_end_to_end_and_the_text_form(readme):
    gorp, data, offsets, ids, caps = readme
    verbs = [b"GET", b"DELETE", b"TRACE", b"GET", b""]
    for keep in (None, "hits", "others"):
        got = check(gorp, data, offsets, ids, caps, VERB_PARTS, verbs, keep=keep, where=[("GetRequest", "timeTakenInMsec", ">=", 100)])
    assert got["entry_same"].tolist() == [0, 1, 2, 0, 4] and got["entry_lines"][0] > 0 and got["entry_lines"][3] == 0
    # membership by path: the paths of the first 300 lines as the dictionary of all 2 000
    first = gorp.group_lines(data[:int(offsets[300])], offsets[:301], ids[:300], caps[:300], [("GetRequest", "path"), ("PutRequest", "path")], keys="csr")
    got = gorp.lookup_lines(data, offsets, ids, caps, [("GetRequest", "path"), ("PutRequest", "path")], first, keep="hits")
    assert np.array_equal(got["line_entry"][:300], first["line_key"]) and got["totals"]["hits"] >= first["totals"]["keyed"]
    assert np.array_equal(got["entry_same"], np.arange(first["totals"]["n_keys"]))
    # the whole-file form: the same lines as text
    text = b"\n".join(bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))) + b"\n"
    for keep in ("hits", "others"):
        batch = check(gorp, data, offsets, ids, caps, VERB_PARTS, verbs, keep=keep)
        res, counts, n_lines = gorp.text_lookup_lines(text, VERB_PARTS, verbs, keep=keep)
        assert n_lines == len(ids) and counts[:3].tolist() == [(ids == k).sum() for k in range(3)]
        for f in ("line_entry", "entry_same", "entry_lines", "entry_first_line", "index"):
            assert np.array_equal(res[f], batch[f]), f
        # the kept lines' ORIGINAL bytes, as gx_text_select writes them: every line with its terminator
        kept = batch["index"].tolist()
        assert res["data"].tobytes() == b"".join(bytes(data[int(offsets[i]):int(offsets[i + 1])]) + b"\n" for i in kept)
        assert res["offsets"].dtype == np.uint32 and np.array_equal(res["offsets"], batch["offsets"] + np.arange(len(kept) + 1, dtype=np.uint32))
        assert res["entry_stats"] == batch["entry_stats"] and res["totals"] == batch["totals"] | {"units_out": batch["totals"]["units_out"] + len(kept)}
