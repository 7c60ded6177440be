"""GPU tests of gx_lines_by_key / gx_text_lines_by_key: every key's lines together, keys in order of their first line, lines in input
order inside each.

Expected values come from tests/by_key_oracle.py -- group_oracle.group_lines for the keys, the keep rule per key,
sorted(kept lines, key=(line_key[i], i)), the two prefixes and the gathered batch -- and everything is compared bit for bit.  Most
batches are fabricated against handles of K identical, trivial extractions with two groups: a line is its key followed by filler, its
capture row (0, |key|, -1, -1) or made up by the test, its id chosen here; the end-to-end cases take ids and rows from gx_extract_batch.
The large shape is compared with a numpy restatement (first-appearance numbering and a stable argsort), which
tests/test_by_key_host.py compares with the oracle on smaller draws of the same generator."""
import ctypes as C

import numpy as np
import pytest

from by_key_oracle import draw, lines_by_key, np_by_key, passes, same
from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, split_lines
from group_oracle import decode_parts
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

BLOCK = 2048                                                             # gx_by_key.hip: BK_BLOCK, and gx_scan.hpp: SCAN_THREADS x SCAN_ITEMS
BY_VERB = [("PutRequest", "verb"), ("GetRequest", "verb"), ("OtherRequest", "verb")]
BY_PATH = [("PutRequest", "path"), ("GetRequest", "path"), ("OtherRequest", "path")]
K0 = [(0, 0)]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, min_lines=1, max_lines=None, where=None, utf8=None, **kw):
    """lines_by_key against the restatement, every field; returns what the call returned."""
    p = gorp.group_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = lines_by_key(data, offsets, ids, caps, decode_parts(p), decode_terms(terms), gorp.num_extractions, min_lines, max_lines)
    got = gorp.lines_by_key(data, offsets, ids, caps, p, min_lines, max_lines, where=terms, utf8=utf8, keys="csr", **kw)
    same(got, want, data.dtype, offsets.dtype)
    return got


_handles = {}


def trivial_handle(K, groups=2):
    """K identical extractions `a(.*)(.*)`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups].num_extractions == K and _handles[K, groups].max_groups == groups
    return _handles[K, groups]


def batch(keys, lengths=None, ids=None, dtype=np.uint8, offsets_dtype=np.uint32):
    """A line is its key (a sequence of code units) and filler up to lengths[i] units (None: the key alone); group 0 is the key, group 1
    unset.  A key of None: the line's key group is unset too."""
    klen = np.array([0 if k is None else len(k) for k in keys], np.int64)
    lens = klen if lengths is None else np.maximum(np.asarray(lengths, np.int64), klen)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(offsets_dtype)
    data = np.full(int(lens.sum()), 0x2E, dtype)
    for i, k in enumerate(keys):
        if k:
            data[int(offsets[i]):int(offsets[i]) + len(k)] = np.frombuffer(k, np.uint8) if isinstance(k, bytes) else k
    caps = np.full((len(keys), 4), -1, np.int32)
    for i, k in enumerate(keys):
        if k is not None:
            caps[i, 0], caps[i, 1] = 0, len(k)
    return data, offsets, np.zeros(len(keys), np.int32) if ids is None else np.asarray(ids, np.int32), caps


def named(names, **kw):
    """batch of keys spelled k<name>; a name below 0: a line whose key group is unset"""
    return batch([None if v < 0 else b"k%d" % v for v in names], **kw)


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


FIELDS = ("index", "bytes", "offsets", "ids", "caps", "kol", "kou")
KEY_FIELDS = ("units", "koff", "first", "lines", "line_key")


def raw_call(gorp, data, offsets, ids, caps, parts, min_lines=1, max_lines=0, cap_lines=0, bytes_cap=0, max_keys=0, units_cap=0, want=FIELDS + KEY_FIELDS, flags=0,
             poison=0xAB, **kw):
    """gx_lines_by_key itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p = gorp.group_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"index": np.zeros(cap_lines + 8, np.uint32), "bytes": np.zeros(bytes_cap + 8, np.uint8), "offsets": np.zeros(cap_lines + 1 + 8, offsets.dtype),
              "ids": np.zeros(cap_lines + 8, np.int32), "caps": np.zeros((cap_lines + 8, 2 * gorp.max_groups), np.int32), "kol": np.zeros(max_keys + 1 + 8, np.uint64),
              "kou": np.zeros(max_keys + 1 + 8, np.uint64), "units": np.zeros(units_cap + 8, data.dtype), "koff": np.zeros(max_keys + 1 + 8, offsets.dtype),
              "first": np.zeros(max_keys + 8, np.uint32), "lines": np.zeros(max_keys + 8, np.uint64), "line_key": np.zeros(n + 8, np.uint32)}
    for k in arrays:
        arrays[k].view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    keys = N.gx_group_out(ptr("units"), units_cap, ptr("koff"), ptr("first"), ptr("lines"), None, ptr("line_key"), max_keys)
    out = N.gx_by_key_out(ptr("index"), ptr("bytes"), ptr("offsets"), ptr("ids"), ptr("caps"), cap_lines, bytes_cap, ptr("kol"), ptr("kou"))
    totals = N.gx_by_key_totals()
    rc = N.lib().gx_lines_by_key(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
                                 None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, None, 0, min_lines, max_lines, flags, C.byref(keys),
                                 C.byref(out) if any(f in want for f in FIELDS) else None, C.byref(totals), C.byref(o))
    return rc, Gorp._by_key_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


# ---------------------------------------------------------------------------
# the edges of a sort workgroup and of a scan block; the copy's chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1])
def test_kept_lines_at_the_edges_of_a_sort_block(m):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(m)
    # m lines of 70 keys (two digits) among unmatched lines and lines whose key group is unset
    keyed = rng.integers(0, min(m, 70), m)
    names = np.full(m + m // 3 + 2, -1, np.int64)
    at = np.sort(rng.permutation(len(names))[:m])
    names[at] = keyed
    ids = np.where(rng.random(len(names)) < 0.5, 0, -1)
    ids[at] = 0
    data, offsets, ids, caps = named(names, lengths=rng.integers(0, 9, len(names)), ids=ids)
    got = check(gorp, data, offsets, ids, caps, K0)
    assert got["totals"]["lines_out"] == m and got["index"].tolist() == sorted(at.tolist(), key=lambda i: (got["line_key"][i], i))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_line_lengths_around_the_copy_chunk(dtype):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(16)
    lengths = rng.permutation(np.repeat([0, 1, 15, 16, 17, 31, 33, 1000], 9))
    # keys of 0 .. 2 units: a line of no units holds the empty key, which is a key like any other
    keys = [bytes(rng.integers(65, 68, min(int(l), int(rng.integers(0, 3)))).astype(np.uint8)) for l in lengths]
    data, offsets, ids, caps = batch(keys, lengths=lengths, dtype=dtype)
    data[:] = rng.integers(1, 250, len(data)).astype(dtype) + (0x300 if dtype == np.uint16 else 0)
    for i, k in enumerate(keys):
        data[int(offsets[i]):int(offsets[i]) + len(k)] = np.frombuffer(k, np.uint8)
    got = check(gorp, data, offsets, ids, caps, K0)
    assert got["totals"]["lines_out"] == len(lengths) and b"" in [bytes(k) for k in keys] and got["totals"]["units_out"] == lengths.sum()
    check(gorp, data, offsets, ids, caps, K0, 9)


# ---------------------------------------------------------------------------
# the digits of the key number
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2, 64, 65, 4096, 4097])
def test_key_counts_at_the_edges_of_a_digit(n_keys):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(n_keys)
    names = np.concatenate([rng.permutation(n_keys), rng.integers(0, n_keys, n_keys // 2 + 3)])
    names = names[rng.permutation(len(names))]
    got = check(gorp, *named(names), K0, max_keys=n_keys)
    assert got["totals"]["n_keys"] == n_keys and passes(n_keys) == {1: 0, 2: 1, 64: 1, 65: 2, 4096: 2, 4097: 3}[n_keys]
    check(gorp, *named(names), K0, 2, max_keys=n_keys)


def test_four_passes_on_2_18_and_one_keys_against_the_numpy_restatement():
    gorp = trivial_handle(1)
    n_keys, n = 2 ** 18 + 1, 300000
    names, extra = draw(n, n_keys, seed=18)
    assert len(np.unique(names[names >= 0])) == n_keys and (names < 0).sum() > 1000             # every name keeps a line; lines without a key among them
    # a line: the name's three bytes and `extra` bytes of filler; no key: unmatched
    lens = 3 + extra
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = np.full(int(offsets[-1]), 0x2E, np.uint8)
    for b in range(3):
        data[offsets[:-1].astype(np.int64) + b] = (np.maximum(names, 0) >> (8 * (2 - b))) & 255
    ids = np.where(names < 0, -1, 0).astype(np.int32)
    caps = np.tile(np.array([0, 3, -1, -1], np.int32), (n, 1))
    for lo, hi in ((1, None), (2, 3)):
        line_key, key_lines, order, kol, kou = np_by_key(names, lens, lo, hi)
        got = gorp.lines_by_key(data, offsets, ids, caps, K0, lo, hi, keys="csr", max_keys=n)
        k = len(key_lines)
        assert got["totals"]["n_keys"] == n_keys == 2 ** 18 + 1 and passes(got["totals"]["n_keys"]) == 4   # the call's own count: four passes, the result in buffer 0
        assert got["totals"]["n_keys"] == k and got["totals"]["lines_out"] == len(order) and got["totals"]["units_out"] == int(kou[-1])
        assert got["totals"]["keys_kept"] == int(np.count_nonzero(np.diff(kol.astype(np.int64))))
        assert np.array_equal(got["line_key"], line_key) and np.array_equal(got["lines"], key_lines) and np.array_equal(got["index"], order)
        assert np.array_equal(got["key_out_lines"], kol) and np.array_equal(got["key_out_units"], kou)
        o64, l64 = offsets.astype(np.int64)[order], lens[order]
        dst = np.concatenate([[0], np.cumsum(l64)])
        assert np.array_equal(got["offsets"], dst.astype(np.uint32))
        src = np.repeat(o64 - dst[:-1], l64) + np.arange(int(dst[-1]))
        assert np.array_equal(got["data"], data[src]) and np.array_equal(got["ids"], ids[order]) and np.array_equal(got["caps"], caps[order])


def test_all_five_digits_give_the_same_bits():
    gorp = trivial_handle(1)
    rng = np.random.default_rng(5)
    names = rng.integers(-1, 700, 5000)
    data, offsets, ids, caps = named(names, lengths=rng.integers(0, 40, 5000))
    plain = check(gorp, data, offsets, ids, caps, K0, 2)
    five = check(gorp, data, offsets, ids, caps, K0, 2, all_digits=True)
    weak = check(gorp, data, offsets, ids, caps, K0, 2, all_digits=True, weak_hash=True)
    for name in ("index", "data", "offsets", "ids", "caps", "key_out_lines", "key_out_units", "line_key", "lines", "key_units"):
        assert plain[name].tobytes() == five[name].tobytes() == weak[name].tobytes(), name


# ---------------------------------------------------------------------------
# stability and skew
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["alternating", "one key", "own keys", "first and last"])
def test_stability_and_skew(shape):
    gorp = trivial_handle(1)
    n = 2 * BLOCK + 77
    names = {"alternating": np.arange(n) & 1, "one key": np.zeros(n, np.int64), "own keys": np.random.default_rng(3).permutation(n),
             "first and last": np.concatenate([[5000], np.arange(n - 2) % 300, [5000]])}[shape]
    got = check(gorp, *named(names, lengths=np.arange(n) % 7 + 6), K0, max_keys=n)
    if shape == "alternating":
        assert got["index"].tolist() == list(range(0, n, 2)) + list(range(1, n, 2))
    if shape == "one key":
        assert got["index"].tolist() == list(range(n)) and got["key_out_lines"].tolist() == [0, n]
    if shape == "own keys":
        assert got["index"].tolist() == list(range(n)) and got["totals"]["keys_kept"] == n       # (keys are numbered by their first line)
    if shape == "first and last":
        assert got["index"][:2].tolist() == [0, n - 1] and got["key_out_lines"][:2].tolist() == [0, 2]


# ---------------------------------------------------------------------------
# lines with no key; the keep rule
# ---------------------------------------------------------------------------
def test_lines_without_a_key_are_dropped_and_counted_and_the_empty_value_is_a_key():
    gorp = trivial_handle(2)
    keys = [b"kx", b"", None, b"kx", b"ky", b"", b"kz", b"kx", b"no", b"kz", b"ky", b"w"]
    #        0      1    2     3      4      5    6      7      8      9      10     11
    ids = [0, 0, 0, -1, 1, 1, -2, 0, 1, 0, -3, 0]          # line 3 unmatched, 6 and 10 exceptions, 2 an unset key group; extraction 1's "no" fails its term
    data, offsets, ids, caps = batch(keys, lengths=[4] * len(keys), ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], where=[(1, 0, "!=", "no")])
    assert got["index"].tolist() == [0, 7, 1, 5, 4, 9, 11] and got["totals"]["unset"] == 1 and got["totals"]["lines"] == 8 and got["totals"]["keyed"] == 7
    assert got["key_offsets"].tolist() == [0, 2, 2, 4, 6, 7]                                    # kx, the empty key, ky, kz, w
    # min_lines = 2 drops the singletons; 1 .. 1 keeps only them -- the orphaned requests; every key is still reported
    twice = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], 2, where=[(1, 0, "!=", "no")])
    assert twice["index"].tolist() == [0, 7, 1, 5] and twice["key_out_lines"].tolist() == [0, 2, 4, 4, 4, 4] and twice["totals"]["keys_kept"] == 2
    once = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], 1, 1, where=[(1, 0, "!=", "no")])
    assert once["index"].tolist() == [4, 9, 11] and once["totals"]["n_keys"] == 5 and once["lines"].tolist() == [2, 2, 1, 1, 1]
    # bounds that keep nothing: both prefixes all zeros, one offset, nothing else written
    for lo, hi in ((3, None), (3, 7), (10 ** 12, None)):
        none = check(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], lo, hi, where=[(1, 0, "!=", "no")])
        assert none["totals"]["lines_out"] == 0 and none["key_out_lines"].tolist() == [0] * 6 == none["key_out_units"].tolist() and none["offsets"].tolist() == [0]
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0), (1, 0)], 3, 0, cap_lines=12, bytes_cap=48, max_keys=6, units_cap=16)
    assert rc == N.GX_OK and totals["lines_out"] == 0 and totals["n_keys"] == 6                 # (no term: "no" is a key too)
    assert untouched({k: arrays[k] for k in ("index", "bytes", "ids", "caps")}) and arrays["offsets"][0] == 0 and (arrays["offsets"].view(np.uint8)[4:] == 0xAB).all()
    assert arrays["kol"][:7].tolist() == [0] * 7 and (arrays["kol"][7:].view(np.uint8) == 0xAB).all() and arrays["lines"][:6].tolist() == [2, 2, 1, 1, 1, 1]
    # no parts, no lines: all zeros
    for args in ((data, offsets, ids, caps, []), (data[:0], offsets[:1], ids[:0], caps[:0], [(0, 0)])):
        got = check(gorp, *args)
        assert got["totals"]["lines_out"] == 0 and got["totals"]["n_keys"] == 0 and got["key_out_lines"].tolist() == [0] and got["offsets"].tolist() == [0]


# ---------------------------------------------------------------------------
# formats and options, each against the int32 / dense run of the same batch
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    n = BLOCK + 300
    names = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 90, n))
    ids = np.where(rng.random(n) < 0.1, rng.integers(-4, 0, n), rng.integers(0, 3, n))
    data, offsets, ids, caps = named(names, lengths=rng.integers(0, 50, n), ids=ids)
    gorp = trivial_handle(3)
    parts = [(0, 0), (2, 0)]
    return gorp, data, offsets, ids, caps, parts, check(gorp, data, offsets, ids, caps, parts, 2, 40)


def test_compact_rows_offsets64_utf16_and_utf8(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    for dtype in (np.uint16, np.uint8):
        rows = pack(ids, caps, dtype)
        got = check(gorp, data, offsets, rows, None, parts, 2, 40)
        assert got["caps"] is None and got["ids"].shape == (len(base["index"]), 5) and np.array_equal(got["ids"], rows[base["index"]])
        assert all(np.array_equal(got[k], base[k]) for k in ("index", "data", "offsets", "key_out_lines", "key_out_units", "line_key"))
    got = check(gorp, data, offsets.astype(np.uint64), ids, caps, parts, 2, 40)
    assert got["offsets"].dtype == np.uint64 and np.array_equal(got["offsets"], base["offsets"]) and np.array_equal(got["index"], base["index"])
    wide = check(gorp, data.astype(np.uint16) | 0x100, offsets, ids, caps, parts, 2, 40)
    assert np.array_equal(wide["data"], base["data"].astype(np.uint16) | 0x100) and np.array_equal(wide["index"], base["index"])
    got = check(gorp, data, offsets, ids, caps, parts, 2, 40, utf8="bytes")
    assert all(np.array_equal(got[k], base[k]) for k in ("index", "data", "offsets", "ids", "caps", "key_out_lines", "key_out_units"))
    got = check(gorp, data, offsets, ids, caps, parts, 2, 40, weak_hash=True)
    assert all(np.array_equal(got[k], base[k]) for k in ("index", "data", "offsets", "ids", "caps", "key_out_lines", "key_out_units", "lines"))


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


def on_device(gorp, d, n, parts, lo, hi, m, units, k, stream=None, **kw):
    """lines_by_key_device with torch buffers, every one poisoned and a little larger than needed.  Returns (rc, totals, host arrays)."""
    import torch
    types = {"index": np.uint32, "data": np.uint8, "offsets": np.uint32, "ids": np.int32, "caps": np.int32, "key_out_lines": np.uint64, "key_out_units": np.uint64,
             "lines": np.uint64, "line_key": np.uint32}
    sizes = {"index": m + 4, "data": units + 64, "offsets": m + 1 + 4, "ids": m + 4, "caps": (m + 4) * 2 * gorp.max_groups, "key_out_lines": k + 1 + 4,
             "key_out_units": k + 1 + 4, "lines": k + 4, "line_key": n + 4}
    t = {name: torch.full((sizes[name] * np.dtype(types[name]).itemsize,), 0x5A, dtype=torch.uint8, device="cuda") for name in types}
    rc, totals = gorp.lines_by_key_device(d["data"].data_ptr(), d["offsets"].data_ptr(), n, d["ids"].data_ptr(), d["caps"].data_ptr(), parts, lo, hi,
                                          key_lines_ptr=t["lines"].data_ptr(), line_key_ptr=t["line_key"].data_ptr(), max_keys=k, out_index_ptr=t["index"].data_ptr(),
                                          out_data_ptr=t["data"].data_ptr(), out_offsets_ptr=t["offsets"].data_ptr(), out_ids_ptr=t["ids"].data_ptr(),
                                          out_caps_ptr=t["caps"].data_ptr(), cap_lines=m, out_bytes_cap=units, key_out_lines_ptr=t["key_out_lines"].data_ptr(),
                                          key_out_units_ptr=t["key_out_units"].data_ptr(), stream=None if stream is None else stream.cuda_stream, **kw)
    if stream is not None:
        stream.synchronize()                                         # (stream order delivers the outputs)
    else:
        torch.cuda.synchronize()
    return rc, totals, {name: v.cpu().numpy().view(types[name]) for name, v in t.items()}


def same_arrays(dev, host, gorp):
    m, k, units = host["totals"]["lines_out"], host["totals"]["n_keys"], host["totals"]["units_out"]
    assert np.array_equal(dev["index"][:m], host["index"]) and np.array_equal(dev["data"][:units], host["data"])
    assert np.array_equal(dev["offsets"][:m + 1], host["offsets"]) and np.array_equal(dev["ids"][:m], host["ids"])
    assert np.array_equal(dev["caps"][:m * 2 * gorp.max_groups].reshape(m, -1), host["caps"])
    assert np.array_equal(dev["key_out_lines"][:k + 1], host["key_out_lines"]) and np.array_equal(dev["key_out_units"][:k + 1], host["key_out_units"])
    assert np.array_equal(dev["lines"][:k], host["lines"]) and np.array_equal(dev["line_key"][:len(host["line_key"])], host["line_key"])
    # nothing behind what the totals say
    for name, used in (("index", m), ("data", units), ("offsets", m + 1), ("ids", m), ("caps", m * 2 * gorp.max_groups), ("key_out_lines", k + 1), ("key_out_units", k + 1),
                       ("lines", k)):
        assert (dev[name][used:].view(np.uint8) == 0x5A).all(), name


def test_device_pointers_streams_and_determinism(mixed, new_stream):
    import torch
    gorp, data, offsets, ids, caps, parts, base = mixed
    n = len(ids)
    d = {"data": torch.from_numpy(data).cuda(), "offsets": torch.from_numpy(offsets.view(np.int32)).cuda(), "ids": torch.from_numpy(ids).cuda(),
         "caps": torch.from_numpy(caps).cuda()}
    m, units, k = base["totals"]["lines_out"], base["totals"]["units_out"], base["totals"]["n_keys"]
    rc, totals, first = on_device(gorp, d, n, parts, 2, 40, m, units, k)
    assert rc == N.GX_OK and totals == base["totals"]
    same_arrays(first, base, gorp)
    # the same call twice, and once more on a stream of the test's own: identical bytes in every output
    rc, totals, second = on_device(gorp, d, n, parts, 2, 40, m, units, k)
    s1, s2 = new_stream(), new_stream()
    torch.cuda.synchronize()
    rc3, totals3, third = on_device(gorp, d, n, parts, 2, 40, m, units, k, stream=s1)
    rc4, totals4, fourth = on_device(gorp, d, n, parts, 2, 40, m, units, k, stream=s2, all_digits=True)
    assert rc == rc3 == rc4 == N.GX_OK and totals == totals3 == totals4 == base["totals"]
    for name in first:
        assert first[name].tobytes() == second[name].tobytes() == third[name].tobytes() == fourth[name].tobytes(), name
    # a capacity one short on the device: nothing written, the totals filled
    for short in (dict(m=m - 1), dict(units=units - 1)):
        sizes = dict(m=m, units=units)
        sizes.update(short)
        rc, totals, dev = on_device(gorp, d, n, parts, 2, 40, sizes["m"], sizes["units"], k)
        assert rc == N.GX_E_LIMIT and totals == base["totals"] and all((a.view(np.uint8) == 0x5A).all() for a in dev.values())


# ---------------------------------------------------------------------------
# capacities
# ---------------------------------------------------------------------------
def test_capacities_the_size_query_and_a_full_table(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    t = base["totals"]
    m, units, k, ku = t["lines_out"], t["units_out"], t["n_keys"], t["key_units"]
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, cap_lines=m, bytes_cap=units, max_keys=k, units_cap=ku)
    assert rc == N.GX_OK and totals == t
    assert np.array_equal(arrays["index"][:m], base["index"]) and np.array_equal(arrays["bytes"][:units], base["data"]) and np.array_equal(arrays["kol"][:k + 1], base["key_out_lines"])
    assert np.array_equal(arrays["caps"][:m], base["caps"]) and np.array_equal(arrays["lines"][:k], base["lines"])
    for name, used in (("index", m), ("bytes", units), ("offsets", m + 1), ("ids", m), ("caps", m), ("kol", k + 1), ("kou", k + 1), ("lines", k), ("units", ku)):
        assert (arrays[name][used:].view(np.uint8) == 0xAB).all(), name
    # one short: GX_E_LIMIT, every output byte of out and of keys still poison, the totals filled
    for short in (dict(cap_lines=m - 1), dict(bytes_cap=units - 1), dict(max_keys=k - 1), dict(units_cap=ku - 1)):
        sizes = dict(cap_lines=m, bytes_cap=units, max_keys=k, units_cap=ku)
        sizes.update(short)
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, **sizes)
        assert rc == N.GX_E_LIMIT and totals == t and untouched(arrays), short
    # the bytes alone need no cap_lines; the per-line outputs alone no bytes_cap
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, bytes_cap=units, max_keys=k, want=("bytes",))
    assert rc == N.GX_OK and np.array_equal(arrays["bytes"][:units], base["data"])
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, cap_lines=m, max_keys=k, want=("index", "offsets", "kou"))
    assert rc == N.GX_OK and np.array_equal(arrays["index"][:m], base["index"]) and np.array_equal(arrays["kou"][:k + 1], base["key_out_units"])
    # the size query delivers the same totals and writes nothing
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, max_keys=k, want=())
    assert rc == N.GX_OK and totals == t and untouched(arrays)
    # max_keys too small for the table itself: exact = 0, as gx_group_lines reports it
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, 2, 40, cap_lines=m, bytes_cap=units, max_keys=16, units_cap=ku)
    assert rc == N.GX_E_LIMIT and not totals["exact"] and totals["n_keys"] == 65 and totals["lines_out"] == 0 and untouched(arrays)
    g_rc, g_totals = gorp.group_lines_device(data.ctypes.data, offsets.ctypes.data, len(ids), ids.ctypes.data, caps.ctypes.data, parts, max_keys=16, device_pointers=False)
    assert g_rc == N.GX_E_LIMIT and all(g_totals[key] == totals[key] for key in g_totals if key != "key_units")   # (not exact: which keys found a slot depends on timing)


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


@pytest.mark.parametrize("parts,lo,hi", [(BY_VERB, 1, None), (BY_VERB, 40, 640), (BY_PATH, 1, None), (BY_PATH, 2, None), (BY_PATH, 1, 1)])
def test_readme_definition_end_to_end(readme, parts, lo, hi):
    gorp, data, offsets, ids, caps = readme
    got = check(gorp, data, offsets, ids, caps, parts, lo, hi)
    assert (got["totals"]["lines_out"] > 0) == any(lo <= c <= (hi or 10 ** 9) for c in got["lines"].tolist())
    # the result is an ordinary batch: extracting it again reproduces the ids and rows that travelled with the lines
    ids2, caps2 = gorp.extract_batch(got["data"], got["offsets"])
    assert np.array_equal(ids2, got["ids"]) and np.array_equal(caps2, got["caps"])
    check(gorp, data, offsets, ids, caps, parts, lo, hi, where=[("GetRequest", "timeTakenInMsec", ">=", 500)])


@pytest.mark.parametrize("last_newline", [True, False])
def test_text_form_equals_the_batch_form_of_its_lines(last_newline):
    gorp = Gorp.construct(W.readme3_definition())
    rng = np.random.default_rng(9)
    verbs = ["GET", "PUT", "POST", "HEAD"]
    lines = ["[%d]: %s %dms /p/%d" % (i, verbs[int(rng.integers(0, 4))], int(rng.integers(0, 900)), int(rng.integers(0, 40))) for i in range(700)]
    lines[13] = "nothing here"
    lines[-1] = "[700]: GET 5ms /p/0"                              # the last line's path was seen before: it lands in the middle
    text = ("\n".join(lines) + ("\n" if last_newline else "")).encode()
    raw = np.frombuffer(text, np.uint8)
    offsets, _ = split_lines(raw)
    n = len(offsets) - 1
    assert n == 700
    ids, caps = gorp.extract_batch(raw, offsets, strip_eol=True)
    for parts, lo, hi in ((BY_VERB, 1, None), (BY_PATH, 2, None), (BY_PATH, 1, 1)):
        want = check(gorp, raw, offsets, ids, caps, parts, lo, hi)
        got, counts, n_lines = gorp.text_lines_by_key(text, parts, lo, hi, keys="csr")
        assert n_lines == n and counts.sum() == n and got["totals"] == want["totals"]
        for name in ("index", "data", "offsets", "key_out_lines", "key_out_units", "line_key", "lines", "first_line", "key_units", "key_offsets"):
            assert np.array_equal(got[name], want[name]), name
        if parts is BY_PATH and lo == 2 and not last_newline:
            j = got["index"].tolist().index(n - 1)
            assert j + 1 < len(got["index"]) and got["data"][got["offsets"][j + 1] - 1] != 10      # the unterminated line, now in the middle


# ---------------------------------------------------------------------------
# the same batch from host buffers and from device pointers
# ---------------------------------------------------------------------------
def twin_batch(n, offsets_dtype):
    """n lines of seven keys; among 65 lines one is empty (its key group unset) and one is unmatched"""
    names, lengths, ids = [i % 7 for i in range(n)], [5 + i % 11 for i in range(n)], [i % 3 for i in range(n)]
    if n > 9:
        names[5], lengths[5] = -1, 0
        names[9], ids[9] = -1, -1
    return named(names, lengths=lengths, ids=ids, offsets_dtype=offsets_dtype)


@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_host_buffers_and_device_pointers_leave_the_same_bytes(n, compact, offsets_dtype):
    from twin_buffers import twins
    gorp = trivial_handle(3)
    data, offsets, ids, caps = twin_batch(n, offsets_dtype)
    if compact:
        ids, caps = pack(ids, caps, np.uint16) if n else np.zeros((0, 5), np.uint16), None
    id_row = ids.itemsize * (ids.shape[1] if ids.ndim == 2 else 1)
    off_w = np.dtype(offsets_dtype).itemsize
    parts = [(0, 0), (1, 0), (2, 0)]
    opts = dict(offsets64=off_w == 8, compact=compact)

    def size_query(b, device_pointers):
        rc, totals = gorp.lines_by_key_device(b.put(data), b.put(offsets), n, b.put(ids), b.put(caps), parts, 2, None, max_keys=n, device_pointers=device_pointers, **opts)
        return rc, totals
    (rc, t), _ = twins(size_query)
    assert rc == N.GX_OK and t["lines_out"] == (n - 2 if n > 9 else 0) and t["n_keys"] == min(n, 7)
    m, units, k = t["lines_out"], t["units_out"], t["n_keys"]

    def call(b, device_pointers):
        rc, totals = gorp.lines_by_key_device(
            b.put(data), b.put(offsets), n, b.put(ids), b.put(caps), parts, 2, None, key_lines_ptr=b.room("lines", k * 8), line_key_ptr=b.room("line_key", n * 4),
            max_keys=n, out_index_ptr=b.room("index", m * 4), out_data_ptr=b.room("data", units), out_offsets_ptr=b.room("offsets", (m + 1) * off_w),
            out_ids_ptr=b.room("ids", m * id_row), out_caps_ptr=None if compact else b.room("caps", m * 16), cap_lines=m, out_bytes_cap=units,
            key_out_lines_ptr=b.room("kol", (k + 1) * 8), key_out_units_ptr=b.room("kou", (k + 1) * 8), device_pointers=device_pointers, **opts)
        return rc, totals
    (rc, totals), rooms = twins(call)
    assert rc == N.GX_OK and totals == t
    index = np.frombuffer(rooms["index"], np.uint32)[:m]
    kept = [i for i in range(n) if n > 9 and i not in (5, 9)]
    first = {}
    for i in kept:
        first.setdefault(i % 7, i)                                     # keys are numbered by their first line
    assert index.tolist() == [i for key in sorted(first, key=first.get) for i in kept if i % 7 == key]
    assert np.frombuffer(rooms["offsets"][:(m + 1) * off_w], offsets_dtype)[m] == units


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

    def size_query(b, device_pointers):
        rc, totals, counts, n_lines = gorp.text_lines_by_key_device(b.put(text16), text.size, BY_PATH, 2, None, max_keys=n, device_pointers=device_pointers)
        return rc, totals, counts.tolist(), n_lines
    (rc, t, counts, n_lines), _ = twins(size_query)
    assert rc == N.GX_OK and n_lines == n and sum(counts) == n and t["lines_out"] == (n - 2 if n > 9 else 0)
    m, units, k = t["lines_out"], t["units_out"], t["n_keys"]

    def call(b, device_pointers):
        rc, totals, counts, n_lines = gorp.text_lines_by_key_device(
            b.put(text16), text.size, BY_PATH, 2, None, key_lines_ptr=b.room("lines", k * 8), line_key_ptr=b.room("line_key", n * 4), max_keys=n,
            out_ptr=b.room("data", units), out_cap=units, out_offsets_ptr=b.room("offsets", (m + 1) * 4), out_index_ptr=b.room("index", m * 4),
            key_out_lines_ptr=b.room("kol", (k + 1) * 8), key_out_units_ptr=b.room("kou", (k + 1) * 8), device_pointers=device_pointers)
        return rc, totals, counts.tolist(), n_lines
    (rc, totals, counts2, _), rooms = twins(call)
    assert rc == N.GX_OK and totals == t and counts2 == counts
    assert len(set(np.frombuffer(rooms["index"], np.uint32)[:m].tolist())) == m and np.frombuffer(rooms["offsets"], np.uint32)[m] == units
