"""GPU tests of gx_sort_lines / gx_text_sort_lines: a whole batch ordered by a number its lines captured, lines without one carried by
the line above them.

Expected values come from tests/sort_oracle.py -- the class rule written out, sorted() over (value, line), the gathered batch -- and
everything is compared bit for bit.  Most batches are fabricated against handles of K identical, trivial extractions with two groups: a
line is its value's text followed by filler, its capture row (0, |value|, -1, -1) or made up by the test, its id chosen here; the
end-to-end cases take ids and rows from gx_extract_batch.  The large shape is compared with a numpy restatement (a forward fill and a
stable argsort), which tests/test_sort_host.py compares with the oracle on smaller draws."""
import ctypes as C

import numpy as np
import pytest

import number_oracle as NO
from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, split_lines
from sort_oracle import CARRIED, REST, STAMPED, decode_parts, np_sort, same, sort_lines
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

BLOCK = 2048                                                             # gx_bucket_sort_dev.hpp: BKT_BLOCK, and gx_scan.hpp: SCAN_THREADS x SCAN_ITEMS
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
K0 = [(0, 0)]
BY_TIME = [("PutRequest", "timeTakenInMsec"), ("GetRequest", "timeTakenInMsec"), ("OtherRequest", "timeTakenInMsec")]
OUTPUTS = ("index", "values", "class", "bytes", "offsets", "ids", "caps")


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, descending=False, carry=False, rest="drop", where=None, utf8=None, formats=None, all_digits=False):
    """sort_lines against the restatement, every field; returns what the call returned."""
    p = gorp.top_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = sort_lines(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions, descending, carry, rest, formats, all_digits)
    got = gorp.sort_lines(data, offsets, ids, caps, p, descending, carry, rest, where=terms, utf8=utf8, all_digits=all_digits)
    same(got, want, data.dtype, offsets.dtype)
    return got


_handles = {}


def trivial_handle(K, groups=2, tag=None):
    """K identical extractions `a(.*)(.*)`: a handle for ids and capture rows made up here (tag: a handle of its own, for formats)."""
    if (K, groups, tag) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups, tag] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups, tag].num_extractions == K and _handles[K, groups, tag].max_groups == groups
    return _handles[K, groups, tag]


def batch(values, lengths=None, ids=None, dtype=np.uint8, offsets_dtype=np.uint32):
    """A line is its value -- an int: its decimal text; bytes: as they are -- and filler up to lengths[i] units (None: the value alone);
    group 0 is the value, group 1 unset.  A value of None: the line's group 0 is unset too."""
    texts = [None if v is None else v if isinstance(v, bytes) else b"%d" % v for v in values]
    tlen = np.array([0 if t is None else len(t) for t in texts], np.int64)
    lens = tlen if lengths is None else np.maximum(np.asarray(lengths, np.int64), tlen)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(offsets_dtype)
    data = np.full(int(lens.sum()), 0x2E, dtype)
    for i, t in enumerate(texts):
        if t:
            data[int(offsets[i]):int(offsets[i]) + len(t)] = np.frombuffer(t, np.uint8)
    caps = np.full((len(texts), 4), -1, np.int32)
    for i, t in enumerate(texts):
        if t is not None:
            caps[i, 0], caps[i, 1] = 0, len(t)
    return data, offsets, np.zeros(len(texts), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


def raw_call(gorp, data, offsets, ids, caps, parts, flags=0, cap_lines=0, bytes_cap=0, want=OUTPUTS, poison=0xAB, **kw):
    """gx_sort_lines itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.top_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"index": np.zeros(cap_lines + 8, np.uint32), "values": np.zeros(cap_lines + 8, np.int64), "class": np.zeros(cap_lines + 8, np.uint8),
              "bytes": np.zeros(bytes_cap + 8, np.uint8), "offsets": np.zeros(cap_lines + 1 + 8, offsets.dtype), "ids": np.zeros(cap_lines + 8, np.int32),
              "caps": np.zeros((cap_lines + 8, 2 * gorp.max_groups), np.int32)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    out = N.gx_sort_out(ptr("index"), ptr("values"), ptr("class"), ptr("bytes"), ptr("offsets"), ptr("ids"), ptr("caps"), cap_lines, bytes_cap)
    totals = N.gx_sort_totals()
    rc = N.lib().gx_sort_lines(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
                               None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, flags, C.byref(out) if want else None,
                               C.byref(totals), C.byref(o))
    return rc, Gorp._sort_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


def on_device(gorp, data, offsets, ids, caps, parts, m, units, stream=None, poison=0x5A, **kw):
    """sort_lines_device with torch buffers, every output poisoned and a little larger than needed.  Returns (rc, totals, host arrays)."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
    d = {"data": up(data), "offsets": up(offsets), "ids": up(ids), "caps": up(caps)}
    id_row = ids.itemsize * (ids.shape[1] if ids.ndim == 2 else 1)
    types = {"index": np.uint32, "values": np.int64, "class": np.uint8, "data": data.dtype, "offsets": offsets.dtype, "ids": ids.dtype, "caps": np.int32}
    sizes = {"index": (m + 4) * 4, "values": (m + 4) * 8, "class": m + 4, "data": (units + 64) * data.itemsize, "offsets": (m + 1 + 4) * offsets.itemsize,
             "ids": (m + 4) * id_row, "caps": (m + 4) * 8 * gorp.max_groups}
    if caps is None:
        del types["caps"]
    t = {name: torch.full((sizes[name],), poison, dtype=torch.uint8, device="cuda") for name in types}
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    rc, totals = gorp.sort_lines_device(ptr(d["data"]), ptr(d["offsets"]), len(offsets) - 1, ptr(d["ids"]), ptr(d["caps"]), parts,
                                        out_index_ptr=t["index"].data_ptr(), out_values_ptr=t["values"].data_ptr(), out_class_ptr=t["class"].data_ptr(),
                                        out_data_ptr=t["data"].data_ptr(), out_offsets_ptr=t["offsets"].data_ptr(), out_ids_ptr=t["ids"].data_ptr(),
                                        out_caps_ptr=t["caps"].data_ptr() if "caps" in t else None, cap_lines=m, out_bytes_cap=units * data.itemsize,
                                        offsets64=offsets.dtype == np.uint64, utf16=data.dtype == np.uint16, compact=gorp._ids_format(ids),
                                        stream=None if stream is None else stream.cuda_stream, **kw)
    if stream is not None:
        stream.synchronize()                                         # (stream order delivers the outputs)
    else:
        torch.cuda.synchronize()
    return rc, totals, {name: v.cpu().numpy().view(types[name]) for name, v in t.items()}


def same_on_device(dev, host, gorp, poison=0x5A):
    """the device call's arrays against Gorp.sort_lines' dict of the same batch: equal, and nothing behind what the totals say"""
    m, units = host["totals"]["lines_out"], host["totals"]["units_out"]
    width = host["ids"].shape[1] if host["ids"].ndim == 2 else 1
    assert np.array_equal(dev["index"][:m], host["index"]) and np.array_equal(dev["values"][:m], host["values"]) and np.array_equal(dev["class"][:m], host["line_class"])
    assert np.array_equal(dev["data"][:units], host["data"]) and np.array_equal(dev["offsets"][:m + 1], host["offsets"])
    assert np.array_equal(dev["ids"][:m * width].reshape(host["ids"].shape), host["ids"])
    used = {"index": m, "values": m, "class": m, "data": units, "offsets": m + 1, "ids": m * width}
    if host["caps"] is not None:
        assert np.array_equal(dev["caps"][:m * 2 * gorp.max_groups].reshape(m, -1), host["caps"])
        used["caps"] = m * 2 * gorp.max_groups
    for name, count in used.items():
        assert (dev[name][count:].view(np.uint8) == poison).all(), name


# ---------------------------------------------------------------------------
# the edges of a sort workgroup and of a scan block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1])
def test_entries_at_the_edges_of_a_sort_block(m):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(m)
    # m stamped lines among unmatched lines and lines whose value group is unset
    n = m + m // 3 + 2
    at = np.sort(rng.permutation(n)[:m])
    values = [None] * n
    for i, v in zip(at, rng.integers(-1000, 1000, m)):
        values[i] = int(v)
    ids = np.where(rng.random(n) < 0.5, 0, -1)
    ids[at] = 0
    data, offsets, ids, caps = batch(values, lengths=rng.integers(0, 9, n), ids=ids)
    got = check(gorp, data, offsets, ids, caps, K0)
    assert got["totals"]["lines_out"] == m == got["totals"]["numbers"] and got["totals"]["rest"] == n - m and sorted(got["index"].tolist()) == at.tolist()
    check(gorp, data, offsets, ids, caps, K0, descending=True)
    got = check(gorp, data, offsets, ids, caps, K0, carry=True, rest="last")
    assert got["totals"]["lines_out"] == n and got["totals"]["carried"] == n - m - int(at[0])


# ---------------------------------------------------------------------------
# the digits of the key
# ---------------------------------------------------------------------------
def shapes():
    rng = np.random.default_rng(4)
    base = 1234567890123
    runs = np.sort(rng.integers(0, 10 ** 6, 700)), np.sort(rng.integers(0, 10 ** 6, 900))
    return {"all equal": ([base] * 300, 0), "digit 10": ([int(k) << 60 for k in rng.integers(-8, 8, 400)], 1),
            "extremes": ([[INT64_MIN, INT64_MAX, 0, -1][int(k)] for k in rng.integers(0, 4, 500)], 11),
            "one middle digit": ([(17 << 36) + (int(k) << 30) + 12345 for k in rng.integers(0, 64, 600)], 1),
            "seven values": ([int(v) for v in rng.integers(0, 7, 5000) * 1000 - 3000], None),
            "ascending": (list(range(-500, 2000)), None), "descending": (list(range(2000, -500, -1)), None),
            "two runs": ([int(v) for v in np.concatenate(runs)], None)}


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shape", list(shapes()))
def test_values_by_the_digits_they_differ_in(shape, descending):
    gorp = trivial_handle(1)
    values, n_passes = shapes()[shape]
    assert shape != "one middle digit" or ({v >> 36 for v in values}, {v & (2 ** 30 - 1) for v in values}) == ({17}, {12345})
    data, offsets, ids, caps = batch(values, lengths=np.arange(len(values)) % 5 + 20)
    plain = check(gorp, data, offsets, ids, caps, K0, descending=descending)
    assert n_passes is None or plain["totals"]["n_passes"] == n_passes
    assert plain["totals"]["already_ordered"] == (shape == "all equal" or shape == ("descending" if descending else "ascending"))
    if shape == "seven values":                                         # stability: every value's lines in input order
        for v in set(values):
            mine = plain["index"][plain["values"] == v].tolist()
            assert mine == sorted(mine) and len(mine) == values.count(v)
    if shape == "all equal":
        assert plain["index"].tolist() == list(range(len(values)))
    eleven = check(gorp, data, offsets, ids, caps, K0, descending=descending, all_digits=True)
    assert eleven["totals"]["n_passes"] == 11
    for name in ("index", "values", "line_class", "data", "offsets", "ids", "caps"):
        assert plain[name].tobytes() == eleven[name].tobytes(), name


# ---------------------------------------------------------------------------
# carried lines and rest lines
# ---------------------------------------------------------------------------
def test_the_first_line_unstamped_and_no_stamped_line_at_all():
    gorp = trivial_handle(1)
    data, offsets, ids, caps = batch([None, 5, None, 3, None], lengths=[3, 4, 0, 6, 2], ids=[0, 0, -1, 0, 0])
    got = check(gorp, data, offsets, ids, caps, K0, carry=True, rest="last")
    assert got["index"].tolist() == [3, 4, 1, 2, 0] and got["line_class"].tolist() == [STAMPED, CARRIED, STAMPED, CARRIED, REST] and got["values"].tolist() == [3, 3, 5, 5, 0]
    assert check(gorp, data, offsets, ids, caps, K0, carry=True)["index"].tolist() == [3, 4, 1, 2]
    # m == 0: with rest last the batch as it came, without nothing but the offsets' one entry
    data, offsets, ids, caps = batch([None, b"x", None, b"-"], lengths=[3, 4, 0, 6], ids=[0, 0, -1, 0])
    for carry in (False, True):
        got = check(gorp, data, offsets, ids, caps, K0, carry=carry, rest="last")
        assert got["index"].tolist() == [0, 1, 2, 3] and got["line_class"].tolist() == [REST] * 4 and got["totals"]["n_passes"] == 0 and got["totals"]["not_numbers"] == 2
        got = check(gorp, data, offsets, ids, caps, K0, carry=carry)
        assert got["totals"]["lines_out"] == 0 and got["offsets"].tolist() == [0] and got["totals"]["rest"] == 4
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, K0, N.GX_SORT_CARRY, cap_lines=4, bytes_cap=16)
    assert rc == N.GX_OK and totals["lines_out"] == 0 and arrays["offsets"][0] == 0 and (arrays["offsets"].view(np.uint8)[4:] == 0xAB).all()
    assert untouched({k: v for k, v in arrays.items() if k != "offsets"})
    # no lines at all
    got = check(gorp, data[:0], offsets[:1], ids[:0], caps[:0], K0, carry=True, rest="last")
    assert got["totals"]["lines_out"] == 0 and got["offsets"].tolist() == [0] and got["totals"]["already_ordered"]


@pytest.mark.parametrize("tail", [300, 2100])
def test_one_stamped_line_carries_a_long_tail(tail):
    gorp = trivial_handle(1)
    # past a 256-lane workgroup and past a 2 048-entry scan block: every carried line reads the one stamped key
    values = [None, None, 7] + [None] * tail + [3, None]
    ids = [0, -1, 0] + [(-1, 0, -2)[i % 3] for i in range(tail)] + [0, -1]
    data, offsets, ids, caps = batch(values, lengths=np.arange(len(values)) % 7, ids=ids)
    got = check(gorp, data, offsets, ids, caps, K0, carry=True, rest="last")
    assert got["index"].tolist() == [tail + 3, tail + 4] + list(range(2, tail + 3)) + [0, 1] and got["totals"]["carried"] == tail + 1
    got = check(gorp, data, offsets, ids, caps, K0, descending=True, carry=True)
    assert got["index"].tolist() == list(range(2, tail + 5)) and got["totals"]["already_ordered"]


def test_carried_lines_of_every_unstamped_kind_and_records_in_both_directions():
    gorp = trivial_handle(3)
    parts = [(0, 0), (2, 0)]
    where = [(0, 0, "!=", "77")]
    #         0 stamped  1 unmatched  2 exception  3 no part  4 failed term  5 unset  6 not a number  7 stamped (r2)  8 zero-length, unmatched  9 stamped
    values = [50,        b"9",        b"9",        9,         77,            None,    b"1x",          -4,             None,                      50]
    ids = [0,            -1,          -2,          1,         0,             0,       0,              2,              -1,                        0]
    data, offsets, ids, caps = batch(values, lengths=[6, 5, 4, 3, 2, 1, 2, 9, 0, 2], ids=ids)
    got = check(gorp, data, offsets, ids, caps, parts, carry=True, where=where)
    assert got["index"].tolist() == [7, 8, 0, 1, 2, 3, 4, 5, 6, 9] and got["line_class"].tolist() == [0, 1, 0, 1, 1, 1, 1, 1, 1, 0]
    assert got["values"].tolist() == [-4, -4] + [50] * 8 and got["totals"]["carried"] == 7 and got["totals"]["rest"] == 0
    assert (got["totals"]["lines"], got["totals"]["numbers"], got["totals"]["unset"], got["totals"]["not_numbers"]) == (5, 3, 1, 1)
    # descending: the records leave in the other order, each still intact and in input order; equal stamps (50, 50) in input order
    got = check(gorp, data, offsets, ids, caps, parts, descending=True, carry=True, where=where)
    assert got["index"].tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 7, 8]
    # without carry they are all rest lines: dropped, or last in input order with value 0 and class 2
    got = check(gorp, data, offsets, ids, caps, parts, where=where)
    assert got["index"].tolist() == [7, 0, 9] and got["totals"]["rest"] == 7
    got = check(gorp, data, offsets, ids, caps, parts, rest="last", where=where)
    assert got["index"].tolist() == [7, 0, 9, 1, 2, 3, 4, 5, 6, 8] and got["values"].tolist()[3:] == [0] * 7 and got["line_class"].tolist()[3:] == [REST] * 7
    check(gorp, data, offsets, ids, caps, parts, descending=True, rest="last", where=where)
    # a leading run that is not stamped stays rest under carry
    lead = batch([b"9", None] + values, lengths=[2, 0, 6, 5, 4, 3, 2, 1, 2, 9, 0, 2], ids=[-1, 0] + ids.tolist())
    got = check(gorp, *lead, parts, carry=True, rest="last", where=where)
    assert got["index"].tolist()[-2:] == [0, 1] and got["totals"]["rest"] == 2 and got["totals"]["carried"] == 7


def test_no_parts_and_rest_last_is_the_identity_copy():
    gorp = trivial_handle(2)
    rng = np.random.default_rng(8)
    n = BLOCK + 17
    data, offsets, ids, caps = batch([int(v) for v in rng.integers(0, 99, n)], lengths=rng.integers(0, 40, n), ids=rng.integers(-2, 2, n))
    for carry in (False, True):
        got = check(gorp, data, offsets, ids, caps, [], carry=carry, rest="last")
        assert got["index"].tolist() == list(range(n)) and np.array_equal(got["data"], data) and np.array_equal(got["offsets"], offsets)
        assert np.array_equal(got["ids"], ids) and np.array_equal(got["caps"], caps) and got["totals"]["rest"] == n and got["totals"]["lines"] == 0
    got = check(gorp, data, offsets, ids, caps, [])
    assert got["totals"]["lines_out"] == 0 and got["totals"]["rest"] == n
    # dense ids without rows: nothing reads them
    got = gorp.sort_lines(data, offsets, ids, None, [], rest="last")
    assert got["caps"] is None and np.array_equal(got["data"], data)


def test_zero_length_lines():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(12)
    n = 700
    values = [None if i % 3 == 0 else int(v) for i, v in enumerate(rng.integers(-5, 5, n))]
    lengths = [0 if v is None else int(rng.integers(2, 30)) for v in values]
    data, offsets, ids, caps = batch(values, lengths=lengths, ids=[0 if i % 6 else -1 for i in range(n)])
    for carry in (False, True):
        got = check(gorp, data, offsets, ids, caps, K0, carry=carry, rest="last")
        assert got["totals"]["units_out"] == sum(lengths) and got["totals"]["lines_out"] == n


# ---------------------------------------------------------------------------
# formats and options, each through host buffers and through device pointers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    n = BLOCK + 300
    values = [None if rng.random() < 0.1 else b"?" if rng.random() < 0.05 else int(rng.integers(-90, 90)) for _ in range(n)]
    ids = np.where(rng.random(n) < 0.1, rng.integers(-4, 0, n), rng.integers(0, 3, n))
    data, offsets, ids, caps = batch(values, lengths=rng.integers(0, 50, n), ids=ids)
    gorp = trivial_handle(3)
    parts = [(0, 0), (2, 0)]
    return gorp, data, offsets, ids, caps, parts, check(gorp, data, offsets, ids, caps, parts, carry=True, rest="last")


def both_ways(gorp, data, offsets, ids, caps, parts, **kw):
    """the call on host buffers, checked against the oracle, and on device pointers, checked against that"""
    host = check(gorp, data, offsets, ids, caps, parts, **kw)
    kw.pop("formats", None)
    where = kw.pop("where", None)
    kw["utf8"] = bool(kw.get("utf8"))
    rc, totals, dev = on_device(gorp, data, offsets, ids, caps, parts, host["totals"]["lines_out"], host["totals"]["units_out"],
                                where=gorp.where_terms(where or [], units=units_of(data, kw["utf8"])), **kw)
    assert rc == N.GX_OK and totals == host["totals"]
    same_on_device(dev, host, gorp)
    return host


def test_compact_rows_offsets64_utf16_and_utf8(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    opt = dict(carry=True, rest="last")
    both_ways(gorp, data, offsets, ids, caps, parts, **opt)
    for dtype in (np.uint16, np.uint8):
        rows = pack(ids, caps, dtype)
        got = both_ways(gorp, data, offsets, rows, None, parts, **opt)
        assert got["caps"] is None and got["ids"].shape == (len(base["index"]), 5) and np.array_equal(got["ids"], rows[base["index"]])
        assert all(np.array_equal(got[k], base[k]) for k in ("index", "values", "line_class", "data", "offsets"))
    got = both_ways(gorp, data, offsets.astype(np.uint64), ids, caps, parts, **opt)
    assert got["offsets"].dtype == np.uint64 and np.array_equal(got["offsets"], base["offsets"]) and np.array_equal(got["index"], base["index"])
    wide = both_ways(gorp, data.astype(np.uint16), offsets, ids, caps, parts, **opt)
    assert np.array_equal(wide["data"], base["data"].astype(np.uint16)) and np.array_equal(wide["index"], base["index"]) and np.array_equal(wide["values"], base["values"])
    got = both_ways(gorp, data, offsets, ids, caps, parts, utf8="bytes", **opt)
    assert all(np.array_equal(got[k], base[k]) for k in ("index", "values", "line_class", "data", "offsets", "ids", "caps"))


def test_where_terms_and_an_iso8601_number_format():
    gorp = trivial_handle(2, tag="iso")
    gorp.set_number_format(0, "v0", "iso8601", 3)
    rng = np.random.default_rng(31)
    stamps = []
    for i in range(900):
        if i % 11 == 5:
            stamps.append(b"  at com.example.Worker.run(Worker.java:%d)" % i)      # a stack trace line: no timestamp
        else:
            stamps.append(b"2024-03-%02dT%02d:%02d:%02d.%03dZ" % tuple(int(x) for x in (rng.integers(1, 29), rng.integers(0, 24), rng.integers(0, 60), rng.integers(0, 60),
                                                                                      rng.integers(0, 1000))))
    data, offsets, ids, caps = batch(stamps, lengths=rng.integers(0, 60, 900), ids=[(0, 0, 0, 1, -1)[i % 5] for i in range(900)])
    formats = {(0, 0): (NO.ISO8601, 3)}
    got = both_ways(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], carry=True, rest="last", formats=formats)
    assert got["totals"]["not_numbers"] > 100 and got["totals"]["numbers"] > 400 and got["totals"]["first_value"] > 1709251200000
    # extraction 1 reads the same group as a long: no stamp is one; terms on the text of the group
    both_ways(gorp, data, offsets, ids, caps, K0, descending=True, carry=True, formats=formats, where=[(0, 0, "startswith", "2024-03-1")])
    both_ways(gorp, data, offsets, ids, caps, K0, formats=formats, where=[(0, 0, "not contains", "T0")])


@pytest.fixture
def new_stream():
    """Streams of the test's own, created and destroyed here, not drawn from torch's pool."""
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


def test_a_second_call_on_another_stream_right_behind_a_device_pointers_call(mixed, new_stream):
    import torch
    gorp, data, offsets, ids, caps, parts, base = mixed
    m, units = base["totals"]["lines_out"], base["totals"]["units_out"]
    other = check(gorp, data, offsets, ids, caps, parts, descending=True)
    s1, s2 = new_stream(), new_stream()
    torch.cuda.synchronize()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
    d = [up(a) for a in (data, offsets, ids, caps)]
    rooms = []
    for stream, kw, want in ((s1, dict(carry=True, rest="last"), base), (s2, dict(descending=True), other)):
        mm, uu = want["totals"]["lines_out"], want["totals"]["units_out"]
        t = {"index": torch.full(((mm + 4) * 4,), 0x5A, dtype=torch.uint8, device="cuda"), "data": torch.full((uu + 64,), 0x5A, dtype=torch.uint8, device="cuda"),
             "values": torch.full(((mm + 4) * 8,), 0x5A, dtype=torch.uint8, device="cuda")}
        # no wait between the two calls: the second call's passes wait for the first call's event, which still reads the workspace
        rc, totals = gorp.sort_lines_device(d[0].data_ptr(), d[1].data_ptr(), len(ids), d[2].data_ptr(), d[3].data_ptr(), parts, out_index_ptr=t["index"].data_ptr(),
                                            out_values_ptr=t["values"].data_ptr(), out_data_ptr=t["data"].data_ptr(), cap_lines=mm, out_bytes_cap=uu,
                                            stream=stream.cuda_stream, **kw)
        assert rc == N.GX_OK and totals == want["totals"]
        rooms.append((t, want))
    s1.synchronize()
    s2.synchronize()
    for t, want in rooms:
        mm, uu = want["totals"]["lines_out"], want["totals"]["units_out"]
        assert np.array_equal(t["index"].cpu().numpy().view(np.uint32)[:mm], want["index"]) and np.array_equal(t["data"].cpu().numpy()[:uu], want["data"])
        assert np.array_equal(t["values"].cpu().numpy().view(np.int64)[:mm], want["values"]) and (t["data"].cpu().numpy()[uu:] == 0x5A).all()
    assert m == len(ids) and units == int(offsets[-1])


# ---------------------------------------------------------------------------
# capacities, the size query, subsets of the outputs
# ---------------------------------------------------------------------------
def test_capacities_the_size_query_and_every_subset_that_leaves_one_output_out(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    flags = N.GX_SORT_CARRY | N.GX_SORT_REST_LAST
    t = base["totals"]
    m, units = t["lines_out"], t["units_out"]
    names = {"index": "index", "values": "values", "class": "line_class", "bytes": "data", "offsets": "offsets", "ids": "ids", "caps": "caps"}
    used = {"index": m, "values": m, "class": m, "bytes": units, "offsets": m + 1, "ids": m, "caps": m}
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, cap_lines=m, bytes_cap=units)
    assert rc == N.GX_OK and totals == t
    for name in OUTPUTS:
        assert np.array_equal(arrays[name][:used[name]], base[names[name]]) and (arrays[name][used[name]:].view(np.uint8) == 0xAB).all(), name
    # one short: GX_E_LIMIT, every output byte still poison, the totals filled -- on host buffers and on device pointers
    for short in (dict(cap_lines=m - 1), dict(bytes_cap=units - 1)):
        sizes = dict(cap_lines=m, bytes_cap=units)
        sizes.update(short)
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, **sizes)
        assert rc == N.GX_E_LIMIT and totals == t and untouched(arrays), short
        rc, totals, dev = on_device(gorp, data, offsets, ids, caps, parts, sizes["cap_lines"], sizes["bytes_cap"], carry=True, rest="last")
        assert rc == N.GX_E_LIMIT and totals == t and all((a.view(np.uint8) == 0x5A).all() for a in dev.values()), short
    # the bytes alone need no cap_lines; the per-line outputs alone no bytes_cap
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, bytes_cap=units, want=("bytes",))
    assert rc == N.GX_OK and np.array_equal(arrays["bytes"][:units], base["data"])
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, cap_lines=m, want=("values", "class"))
    assert rc == N.GX_OK and np.array_equal(arrays["values"][:m], base["values"]) and np.array_equal(arrays["class"][:m], base["line_class"])
    # every subset that leaves one output out: the others as ever, the one left out untouched
    for out in OUTPUTS:
        want = tuple(x for x in OUTPUTS if x != out)
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, cap_lines=m, bytes_cap=units, want=want)
        assert rc == N.GX_OK and totals == t and untouched({out: arrays[out]}), out
        for name in want:
            assert np.array_equal(arrays[name][:used[name]], base[names[name]]) and (arrays[name][used[name]:].view(np.uint8) == 0xAB).all(), (out, name)
    # the size query -- out NULL, or all of its pointers NULL -- delivers the same totals and writes nothing
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, flags, want=())
    assert rc == N.GX_OK and totals == t and untouched(arrays)
    rc, totals = gorp.sort_lines_device(data.ctypes.data, offsets.ctypes.data, len(ids), ids.ctypes.data, caps.ctypes.data, parts, carry=True, rest="last",
                                        cap_lines=0, device_pointers=False)
    assert rc == N.GX_OK and totals == t


# ---------------------------------------------------------------------------
# the README definition, extracted for real: agreement with gx_top_lines
# ---------------------------------------------------------------------------
def test_agreement_with_top_lines_on_an_extracted_batch():
    gorp = Gorp.construct(W.readme3_definition())
    n = 20000
    t_data, _, cat = W.readme3_lines(n, seed=5)
    data = t_data.numpy().copy()
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(ids, cat.numpy().astype(np.int32))
    for descending in (True, False):
        got = gorp.sort_lines(data, offsets, ids, caps, BY_TIME, descending=descending)
        index, values, data2, off2, ids2, rows2, totals = gorp.top_lines(data, offsets, ids, caps, BY_TIME, 4096, largest=descending)
        assert totals["n_top"] == 4096 and got["totals"]["lines_out"] == totals["numbers"] > 4096
        assert np.array_equal(got["index"][:4096], index) and np.array_equal(got["values"][:4096], values)
        assert np.array_equal(got["data"][:len(data2)], data2) and np.array_equal(got["offsets"][:4097], off2) and np.array_equal(got["ids"][:4096], ids2)
        assert np.array_equal(got["caps"][:4096], rows2)
        assert all(got["totals"][k] == totals[k] for k in ("lines", "numbers", "unset", "not_numbers"))
        steps = np.diff(got["values"])
        assert (steps <= 0).all() if descending else (steps >= 0).all()
        # the result is an ordinary batch: extracting it again reproduces the ids and rows that travelled with the lines
        ids3, caps3 = gorp.extract_batch(got["data"], got["offsets"])
        assert np.array_equal(ids3, got["ids"]) and np.array_equal(caps3, got["caps"])


@pytest.mark.parametrize("last_newline", [True, False])
def test_text_form_equals_the_batch_form_of_its_lines(last_newline):
    gorp = Gorp.construct(W.readme3_definition())
    rng = np.random.default_rng(9)
    verbs = ["GET", "PUT", "POST", "HEAD"]
    lines = ["[%d]: %s %dms /p/%d" % (i, verbs[int(rng.integers(0, 4))], int(rng.integers(100, 900)), int(rng.integers(0, 40))) for i in range(700)]
    lines[13] = "nothing here"
    lines[40] = "\tat some.Frame(of.a.trace)"
    lines[-1] = "[700]: GET 500ms /p/0"                            # the last line sorts to the middle
    text = ("\n".join(lines) + ("\n" if last_newline else "")).encode()
    raw = np.frombuffer(text, np.uint8)
    offsets, _ = split_lines(raw)
    n = len(offsets) - 1
    assert n == 700
    ids, caps = gorp.extract_batch(raw, offsets, strip_eol=True)
    for kw in (dict(), dict(carry=True), dict(descending=True, carry=True, rest="last"), dict(rest="last", where=[("GetRequest", "timeTakenInMsec", ">=", 500)])):
        want = check(gorp, raw, offsets, ids, caps, BY_TIME, **kw)
        got, counts, n_lines = gorp.text_sort_lines(text, BY_TIME, **kw)
        assert n_lines == n and counts.sum() == n and got["totals"] == want["totals"]
        for name in ("index", "values", "line_class", "data", "offsets"):
            assert np.array_equal(got[name], want[name]), name
        if not kw:
            j = got["index"].tolist().index(n - 1)
            assert 0 < j and j + 1 < len(got["index"]) and (got["data"][got["offsets"][j + 1] - 1] != 10) == (not last_newline)   # the unterminated line, now in the middle
    # on device pointers the same bytes
    import torch
    text16 = np.zeros((raw.size + 15) // 16 * 16 + 16, np.uint8)       # (a device text is 16-byte aligned: torch's allocations are)
    text16[:raw.size] = raw
    want, _, _ = gorp.text_sort_lines(text, BY_TIME, carry=True, rest="last")
    m, units = want["totals"]["lines_out"], want["totals"]["units_out"]
    d = torch.from_numpy(text16).cuda()
    t = {name: torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda") for name, size in (("data", units), ("offsets", 4 * (m + 1)), ("index", 4 * m),
                                                                                                  ("values", 8 * m), ("class", m))}
    rc, totals, counts, n_lines = gorp.text_sort_lines_device(d.data_ptr(), raw.size, BY_TIME, carry=True, rest="last", out_ptr=t["data"].data_ptr(), out_cap=units,
                                                              out_offsets_ptr=t["offsets"].data_ptr(), out_index_ptr=t["index"].data_ptr(),
                                                              out_values_ptr=t["values"].data_ptr(), out_class_ptr=t["class"].data_ptr())
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals == want["totals"] and n_lines == n
    host = {name: v.cpu().numpy() for name, v in t.items()}
    assert np.array_equal(host["data"][:units], want["data"]) and np.array_equal(host["offsets"][:4 * (m + 1)].view(np.uint32), want["offsets"])
    assert np.array_equal(host["index"][:4 * m].view(np.uint32), want["index"]) and np.array_equal(host["values"][:8 * m].view(np.int64), want["values"])
    assert np.array_equal(host["class"][:m], want["line_class"]) and all((host[k][-16:] == 0x5A).all() for k in host)
    # out_cap one short: nothing written
    rc, totals, _, _ = gorp.text_sort_lines_device(raw.ctypes.data, raw.size, BY_TIME, carry=True, rest="last", out_ptr=text16.ctypes.data, out_cap=units - 1,
                                                   device_pointers=False)
    assert rc == N.GX_E_LIMIT and totals == want["totals"] and np.array_equal(text16[:raw.size], raw)


# ---------------------------------------------------------------------------
# the large shape
# ---------------------------------------------------------------------------
def test_a_million_lines_against_the_numpy_restatement():
    gorp = trivial_handle(1)
    n, width, digits = 1 << 20, 64, 12
    rng = np.random.default_rng(1)
    # timestamps of two interleaved sources that drift apart, a quarter of the lines without one (unmatched)
    numbers = (np.arange(n, dtype=np.int64) * 1000 + rng.integers(0, 3 * 10 ** 6, n)) % 10 ** digits
    stamped = rng.random(n) >= 0.25
    stamped[:3], stamped[3] = False, True
    data = np.full((n, width), 0x2E, np.uint8)
    rest = numbers.copy()
    for c in range(digits - 1, -1, -1):
        data[:, c] = 0x30 + rest % 10
        rest //= 10
    data = data.reshape(-1)
    offsets = (np.arange(n + 1, dtype=np.uint64) * width).astype(np.uint32)
    ids = np.where(stamped, 0, -1).astype(np.int32)
    caps = np.tile(np.array([0, digits, -1, -1], np.int32), (n, 1))
    for kw in (dict(carry=True, rest="last"), dict(descending=True)):
        index, values, cls = np_sort(numbers, stamped, kw.get("carry", False), kw.get("descending", False), kw.get("rest") == "last")
        got = gorp.sort_lines(data, offsets, ids, caps, K0, **kw)
        m = len(index)
        assert got["totals"]["lines_out"] == m and got["totals"]["numbers"] == int(stamped.sum()) and got["totals"]["units_out"] == m * width
        assert got["totals"]["rest"] == (3 if kw.get("carry") else n - int(stamped.sum())) and not got["totals"]["already_ordered"]
        assert np.array_equal(got["index"], index) and np.array_equal(got["values"], values) and np.array_equal(got["line_class"], cls)
        assert np.array_equal(got["offsets"], (np.arange(m + 1, dtype=np.uint64) * width).astype(np.uint32))
        assert np.array_equal(got["data"].reshape(m, width), data.reshape(n, width)[index]) and np.array_equal(got["ids"], ids[index])
        assert np.array_equal(got["caps"], caps[index])
