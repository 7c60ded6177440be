"""GPU tests of gx_group_pairs / gx_text_group_pairs: the lines of a batch grouped by two captured texts -- the pairs (key, second) in
order of their first line, the lines and the first line of every pair, the pairs of every key, the pair of every line.

Expected values come from tests/pairs_oracle.py -- group_oracle.group_lines for the keys, then a dict keyed by (line_key[i], second)
filled line by line -- and everything is compared bit for bit; the key outputs are also compared with gx_group_lines on the same
batch.  Most batches are fabricated against handles of K identical, trivial extractions with two groups: a line is its key, its second
and filler, its capture row (0, |key|, |key|, |key| + |second|) or made up by the test, its id chosen here; the end-to-end cases take
ids and rows from gx_extract_batch.  The large shapes are compared with a numpy restatement (first-appearance numbering by a
minimum-scatter), which tests/test_pairs_host.py compares with the oracle on smaller draws of the same generator."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, split_lines
from group_oracle import decode_parts
from pairs_oracle import batch, decode_seconds, draw, group_pairs, named_batch, np_pairs, same
from where_oracle import decode_terms, unpack

pytestmark = pytest.mark.gpu

BLOCK = 2048                                                             # gx_scan.hpp: SCAN_THREADS x SCAN_ITEMS
GROUP_LDS_KEYS = 64                                                      # gx_group.hpp
P0 = [(0, 0, 1)]                                                         # extraction 0: group 0 the key, group 1 the second
KEY_FIELDS = ("key_units", "key_offsets", "first_line", "lines", "line_key")
PAIR_FIELDS = ("pair_units", "pair_offsets", "pair_key", "pair_first_line", "pair_lines", "key_pairs", "line_pair")
VERB_PATH = [("PutRequest", "verb", "path"), ("GetRequest", "verb", "path"), ("OtherRequest", "verb", "path")]
VERB_MSEC = [("PutRequest", "verb", "timeTakenInMsec"), ("GetRequest", "verb", "timeTakenInMsec"), ("OtherRequest", "verb", "timeTakenInMsec")]


def units_of(data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check(gorp, data, offsets, ids, caps, parts, where=None, utf8=None, **kw):
    """group_pairs against the restatement, every field, and its key outputs against group_lines on the same batch; returns what the
    call returned."""
    p, s = gorp.pair_parts(parts)
    terms = gorp.where_terms(where or [], units=units_of(data, utf8))
    want = group_pairs(data, offsets, ids, caps, decode_parts(p), decode_seconds(s, p.n), decode_terms(terms), gorp.num_extractions)
    got = gorp.group_pairs(data, offsets, ids, caps, (p, s), where=terms, utf8=utf8, keys="csr", **kw)
    same(got, want, data.dtype, offsets.dtype)
    alone = gorp.group_lines(data, offsets, ids, caps, p, where=terms, utf8=utf8, keys="csr", **{k: v for k, v in kw.items() if k in ("max_keys", "weak_hash")})
    for name in KEY_FIELDS:
        assert got[name].dtype == alone[name].dtype and got[name].tobytes() == alone[name].tobytes(), name
    assert all(got["totals"][k] == v for k, v in alone["totals"].items()) and got["stats"] == alone["stats"]
    return got


_handles = {}


def trivial_handle(K, groups=2):
    """K identical extractions `a(.*)(.*)`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups].num_extractions == K and _handles[K, groups].max_groups == groups
    return _handles[K, groups]


def named(kn, sn, **kw):
    """batch of keys spelled k<name> and seconds spelled s<name>; a name below 0: that group is unset"""
    return batch([None if v < 0 else b"k%d" % v for v in kn], [None if v < 0 else b"s%d" % v for v in sn], **kw)


def pack(ids, caps, dtype):
    """u16 / u8 result rows of int32 ids and dense rows (gx_layout.hpp): -1 becomes the all-ones unit"""
    rows = (np.concatenate([np.asarray(ids)[:, None].astype(np.int64), np.asarray(caps).astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


# ---------------------------------------------------------------------------
# what a pair is
# ---------------------------------------------------------------------------
def test_two_texts_one_behind_the_other_are_no_key():
    gorp = trivial_handle(1)
    got = check(gorp, *batch([b"ab", b"a", b"ab", b"a"], [b"c", b"bc", b"c", b"bc"]), P0)
    assert got["totals"]["n_pairs"] == 2 and got["pair_key"].tolist() == [0, 1] and got["pair_lines"].tolist() == [2, 2] and got["line_pair"].tolist() == [0, 1, 0, 1]
    got = check(gorp, *batch([b"a", b"b", b"a", b"b"], [b"b", b"a", b"b", b"a"]), P0)
    assert got["totals"]["n_pairs"] == 2 and bytes(got["pair_units"]) == b"ba" and got["key_pairs"].tolist() == [1, 1]
    # the same second under two keys: two pairs; two seconds under one key: two pairs of that key
    got = check(gorp, *batch([b"x", b"y", b"x", b"x"], [b"s", b"s", b"s", b"t"]), P0)
    assert got["pair_key"].tolist() == [0, 1, 0] and got["pair_lines"].tolist() == [2, 1, 1] and got["key_pairs"].tolist() == [2, 1]


def test_the_same_pair_captured_by_two_parts_is_one_pair():
    gorp = trivial_handle(3)
    data, offsets, ids, caps = batch([b"k", b"k", b"k", b"q", b"k"], [b"s", b"s", b"s", b"s", b"s"], ids=[0, 2, 1, 2, -1])
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (2, 0, 1)])
    assert got["totals"]["n_pairs"] == 2 and got["pair_lines"].tolist() == [2, 1] and got["line_pair"].tolist() == [0, 0, 0xFFFFFFFF, 1, 0xFFFFFFFF]
    # the parts in the other order, and extraction 2's groups the other way round: its lines key on the text "s"
    caps2 = caps.copy()
    caps2[ids == 2] = caps[ids == 2][:, [2, 3, 0, 1]]
    got = check(gorp, data, offsets, ids, caps2, [(2, 0, 1), (0, 0, 1)])
    assert got["totals"]["n_pairs"] == 3 and got["totals"]["n_keys"] == 2               # ("k","s"), ("s","k") and ("s","q")


def test_the_empty_second_an_unset_second_and_a_part_without_a_second():
    gorp = trivial_handle(2)
    keys = [b"k", b"k", b"k", b"k", b"k", None, b"k"]
    seconds = [b"", None, b"x", b"", b"x", b"x", b""]
    ids = [0, 0, 1, 0, 0, 0, 1]
    data, offsets, ids, caps = batch(keys, seconds, lengths=[3] * 7, ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (1, 0, None)])
    # extraction 1's lines have a key and no second; line 1's second is unset; line 5 has no key at all
    assert got["totals"]["keyed"] == 6 and got["totals"]["paired"] == 3 and got["totals"]["unpaired"] == 3 and got["totals"]["unset"] == 1
    assert got["pair_offsets"].tolist() == [0, 0, 1] and got["pair_lines"].tolist() == [2, 1] and got["line_pair"].tolist() == [0, NONE, NONE, 0, 1, NONE, NONE]
    assert got["key_pairs"].tolist() == [2]


NONE = 0xFFFFFFFF


def test_a_malformed_second_is_never_dereferenced_and_counts_as_unpaired():
    gorp = trivial_handle(1)
    n = 70
    data, offsets, ids, caps = batch([b"key"] * n, [b"sec"] * n, lengths=[8] * n)
    bad = [(5, 3), (3, 9), (-1, 2), (-5, -1), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 5), (7, 2 ** 31 - 1), (9, 9)]
    for q, (b, e) in enumerate(bad):
        caps[3 + 7 * q, 2:] = (b, e)
    caps[69, 2:] = (8, 8)                                   # the empty second at the very end of the last line is a value
    got = check(gorp, data, offsets, ids, caps, P0)
    assert got["totals"]["unpaired"] == len(bad) and got["totals"]["n_pairs"] == 2 and got["pair_offsets"].tolist() == [0, 3, 3]
    assert [i for i, p in enumerate(got["line_pair"].tolist()) if p == NONE] == [3 + 7 * q for q in range(len(bad))]


# ---------------------------------------------------------------------------
# the edges of the machinery
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1])
def test_line_counts_at_the_edges_of_a_wave_a_workgroup_and_a_scan_block(n):
    gorp = trivial_handle(2)
    rng = np.random.default_rng(n)
    kn, sn = rng.integers(-1, 9, n), rng.integers(-1, 7, n)
    ids = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n))
    ids[n - 1], kn[n - 1], sn[n - 1] = 0, 8, 6                       # the last line holds a pair of its own... mostly
    data, offsets, ids, caps = named(kn, sn, lengths=rng.integers(0, 12, n), ids=ids)
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1), (1, 0, 1)])
    assert got["line_pair"][n - 1] != NONE and got["totals"]["paired"] + got["totals"]["unpaired"] == got["totals"]["keyed"]


def test_the_grid_strides_second_trip():
    gorp = trivial_handle(1)
    n = 256 * 2048 + 1
    kn, sn, _ = draw(n, 300, 40, seed=3)
    kn[n - 1], sn[n - 1] = 299, 39
    extra = np.where(sn < 0, -1, np.random.default_rng(4).integers(0, 2, n))   # lines of 2 to 4 bytes
    data, offsets, ids, caps = named_batch(kn, sn, extra)
    line_key, key_lines, line_pair, pair_key, pair_first, pair_lines, key_pairs = np_pairs(kn, sn, 40)
    got = gorp.group_pairs(data, offsets, ids, caps, P0, keys="csr", max_keys=1024, max_pairs=16384)
    assert got["totals"]["n_pairs"] == len(pair_key) and got["totals"]["paired"] == int(pair_lines.sum()) and got["line_pair"][n - 1] != NONE
    for name, want in (("line_key", line_key), ("lines", key_lines), ("line_pair", line_pair), ("pair_key", pair_key), ("pair_first_line", pair_first),
                       ("pair_lines", pair_lines), ("key_pairs", key_pairs)):
        assert got[name].dtype == want.dtype and np.array_equal(got[name], want), name
    assert np.array_equal(got["pair_units"], (sn[pair_first.astype(np.int64)] & 255).astype(np.uint8)) and np.array_equal(got["pair_offsets"], np.arange(len(pair_key) + 1))


@pytest.mark.parametrize("shape", ["one pair", "64 pairs", "two keys one second", "two keys two seconds", "one key 64 seconds"])
def test_the_64_lanes_of_a_wave(shape):
    gorp = trivial_handle(1)
    lane = np.arange(64)
    kn, sn = {"one pair": (lane * 0, lane * 0), "64 pairs": (lane, lane), "two keys one second": (lane & 1, lane * 0), "two keys two seconds": (lane & 1, (lane >> 1) & 1),
              "one key 64 seconds": (lane * 0, lane)}[shape]
    for waves in (1, 3):
        got = check(gorp, *named(np.tile(kn, waves), np.tile(sn, waves)), P0)
        assert got["totals"]["n_pairs"] == {"one pair": 1, "64 pairs": 64, "two keys one second": 2, "two keys two seconds": 4, "one key 64 seconds": 64}[shape]
        assert set(got["pair_lines"].tolist()) == {64 * waves // got["totals"]["n_pairs"]}


@pytest.mark.parametrize("shape", ["one key 200 seconds", "200 keys", "200 keys 2 seconds"])
def test_more_pairs_and_keys_in_a_workgroup_than_its_lds_table_holds(shape):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(7)
    n = 3 * 256
    q = rng.integers(0, 200, n)
    kn, sn = {"one key 200 seconds": (q * 0, q), "200 keys": (q, q * 0), "200 keys 2 seconds": (q, rng.integers(0, 2, n))}[shape]
    got = check(gorp, *named(kn, sn), P0)
    assert got["totals"]["n_pairs"] > 2 * GROUP_LDS_KEYS and int(got["pair_lines"].sum()) == n


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_second_lengths_around_the_copy_step(dtype):
    gorp = trivial_handle(1)
    rng = np.random.default_rng(16)
    lengths = rng.permutation(np.repeat([0, 1, 63, 64, 65, 300], 5))
    top = 250 if dtype == np.uint8 else 0xFFF0
    seconds = [rng.integers(1, top, int(l)).astype(dtype) for l in lengths]
    keys = [rng.integers(65, 68, int(rng.integers(0, 3))).astype(dtype) for _ in lengths]
    got = check(gorp, *batch(keys, seconds, lengths=lengths + rng.integers(0, 9, len(lengths)), dtype=dtype), P0)
    assert set(np.diff(got["pair_offsets"].astype(np.int64)).tolist()) == {0, 1, 63, 64, 65, 300}


def test_the_weak_hash_gives_the_same_bits():
    gorp = trivial_handle(2)
    rng = np.random.default_rng(5)
    n = 3000
    kn, sn = rng.integers(-1, 30, n), rng.integers(-1, 25, n)
    data, offsets, ids, caps = named(kn, sn, lengths=rng.integers(0, 20, n), ids=rng.integers(-1, 2, n))
    parts = [(0, 0, 1), (1, 0, 1)]
    strong = check(gorp, data, offsets, ids, caps, parts)
    weak = check(gorp, data, offsets, ids, caps, parts, weak_hash=True)
    assert strong["totals"]["n_pairs"] > 300 and strong["totals"] == weak["totals"]
    for name in KEY_FIELDS + PAIR_FIELDS:
        assert strong[name].tobytes() == weak[name].tobytes(), name


# ---------------------------------------------------------------------------
# formats and options, each against the int32 / dense run of the same batch
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    n = BLOCK + 300
    kn = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 40, n))
    sn = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 30, n))
    ids = np.where(rng.random(n) < 0.1, rng.integers(-4, 0, n), rng.integers(0, 3, n))
    data, offsets, ids, caps = named(kn, sn, lengths=rng.integers(0, 50, n), ids=ids)
    gorp = trivial_handle(3)
    parts = [(0, 0, 1), (2, 0, 1)]
    return gorp, data, offsets, ids, caps, parts, check(gorp, data, offsets, ids, caps, parts)


def test_compact_rows_offsets64_utf16_utf8_and_terms(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    for dtype in (np.uint16, np.uint8):
        got = check(gorp, data, offsets, pack(ids, caps, dtype), None, parts)
        assert all(np.array_equal(got[k], base[k]) for k in KEY_FIELDS + PAIR_FIELDS)
    got = check(gorp, data, offsets.astype(np.uint64), ids, caps, parts)
    assert got["pair_offsets"].dtype == np.uint64 and np.array_equal(got["pair_offsets"], base["pair_offsets"]) and np.array_equal(got["line_pair"], base["line_pair"])
    wide = check(gorp, data.astype(np.uint16) | 0x100, offsets, ids, caps, parts)
    assert np.array_equal(wide["pair_units"], base["pair_units"].astype(np.uint16) | 0x100) and np.array_equal(wide["line_pair"], base["line_pair"])
    got = check(gorp, data, offsets, ids, caps, parts, utf8="bytes")
    assert all(np.array_equal(got[k], base[k]) for k in KEY_FIELDS + PAIR_FIELDS)
    # terms: the lines that fail one neither count nor pair
    got = check(gorp, data, offsets, ids, caps, parts, where=[(0, 1, "!=", "s3"), (2, 0, "startswith", "k1")])
    assert 0 < got["totals"]["n_pairs"] < base["totals"]["n_pairs"] and got["totals"]["lines"] < base["totals"]["lines"]
    # a part with a value group beside its second: the stats are gx_group_lines'
    got = check(gorp, data, offsets, ids, caps, [(0, 0, 1, 1), (2, 0, 1)])
    assert got["stats"] is not None and np.array_equal(got["line_pair"], base["line_pair"])


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


DEV_TYPES = {"key_units": np.uint8, "key_offsets": np.uint32, "first_line": np.uint32, "lines": np.uint64, "line_key": np.uint32, "pair_units": np.uint8,
             "pair_offsets": np.uint32, "pair_key": np.uint32, "pair_first_line": np.uint32, "pair_lines": np.uint64, "key_pairs": np.uint64, "line_pair": np.uint32}


def on_device(gorp, d, n, parts, k, ku, p, pu, stream=None, **kw):
    """group_pairs_device with torch buffers, every one poisoned and a little larger than needed.  Returns (rc, totals, host arrays)."""
    import torch
    sizes = {"key_units": ku + 16, "key_offsets": k + 1 + 4, "first_line": k + 4, "lines": k + 4, "line_key": n + 4, "pair_units": pu + 16, "pair_offsets": p + 1 + 4,
             "pair_key": p + 4, "pair_first_line": p + 4, "pair_lines": p + 4, "key_pairs": k + 4, "line_pair": n + 4}
    t = {name: torch.full((sizes[name] * np.dtype(DEV_TYPES[name]).itemsize,), 0x5A, dtype=torch.uint8, device="cuda") for name in DEV_TYPES}
    rc, totals = gorp.group_pairs_device(d["data"].data_ptr(), d["offsets"].data_ptr(), n, d["ids"].data_ptr(), d["caps"].data_ptr(), parts,
                                         key_units_ptr=t["key_units"].data_ptr(), key_units_cap=ku, key_offsets_ptr=t["key_offsets"].data_ptr(),
                                         key_first_line_ptr=t["first_line"].data_ptr(), key_lines_ptr=t["lines"].data_ptr(), line_key_ptr=t["line_key"].data_ptr(),
                                         max_keys=k, pair_units_ptr=t["pair_units"].data_ptr(), pair_units_cap=pu, pair_offsets_ptr=t["pair_offsets"].data_ptr(),
                                         pair_key_ptr=t["pair_key"].data_ptr(), pair_first_line_ptr=t["pair_first_line"].data_ptr(),
                                         pair_lines_ptr=t["pair_lines"].data_ptr(), key_pairs_ptr=t["key_pairs"].data_ptr(), line_pair_ptr=t["line_pair"].data_ptr(),
                                         max_pairs=p, stream=None if stream is None else stream.cuda_stream, **kw)
    if stream is not None:
        stream.synchronize()                                         # (stream order delivers the outputs)
    else:
        torch.cuda.synchronize()
    return rc, totals, {name: v.cpu().numpy().view(DEV_TYPES[name]) for name, v in t.items()}


def test_device_pointers_streams_and_repeatability(mixed, new_stream):
    import torch
    gorp, data, offsets, ids, caps, parts, base = mixed
    n = len(ids)
    d = {"data": torch.from_numpy(data).cuda(), "offsets": torch.from_numpy(offsets.view(np.int32)).cuda(), "ids": torch.from_numpy(ids).cuda(),
         "caps": torch.from_numpy(caps).cuda()}
    t = base["totals"]
    k, ku, p, pu = t["n_keys"], t["key_units"], t["n_pairs"], t["pair_units"]
    rc, totals, first = on_device(gorp, d, n, parts, k, ku, p, pu)
    assert rc == N.GX_OK and totals == t
    used = {"key_units": ku, "key_offsets": k + 1, "first_line": k, "lines": k, "line_key": n, "pair_units": pu, "pair_offsets": p + 1, "pair_key": p,
            "pair_first_line": p, "pair_lines": p, "key_pairs": k, "line_pair": n}
    for name, m in used.items():
        assert np.array_equal(first[name][:m], base[name]), name
        assert (first[name][m:].view(np.uint8) == 0x5A).all(), name          # nothing behind what the totals say
    # the same call three times in one process, then on streams of the test's own: identical bytes in every output
    rc2, totals2, second = on_device(gorp, d, n, parts, k, ku, p, pu)
    rc3, totals3, third = on_device(gorp, d, n, parts, k, ku, p, pu)
    s1, s2 = new_stream(), new_stream()
    torch.cuda.synchronize()
    rc4, totals4, fourth = on_device(gorp, d, n, parts, k, ku, p, pu, stream=s1)
    rc5, totals5, fifth = on_device(gorp, d, n, parts, k, ku, p, pu, stream=s2, weak_hash=True)
    assert rc2 == rc3 == rc4 == rc5 == N.GX_OK and totals2 == totals3 == totals4 == totals5 == t
    for name in first:
        assert first[name].tobytes() == second[name].tobytes() == third[name].tobytes() == fourth[name].tobytes() == fifth[name].tobytes(), name
    # a capacity one short on the device: nothing written, the totals filled
    for short in (dict(p=p - 1), dict(pu=pu - 1), dict(k=k - 1)):
        sizes = dict(k=k, ku=ku, p=p, pu=pu)
        sizes.update(short)
        rc, totals, dev = on_device(gorp, d, n, parts, **sizes)
        assert rc == N.GX_E_LIMIT and totals == t and all((a.view(np.uint8) == 0x5A).all() for a in dev.values()), short


# ---------------------------------------------------------------------------
# capacities
# ---------------------------------------------------------------------------
RAW = {"units": "key_units", "koff": "key_offsets", "first": "first_line", "lines": "lines", "line_key": "line_key"}


def raw_call(gorp, data, offsets, ids, caps, parts, max_keys=0, units_cap=0, max_pairs=0, pair_units_cap=0, want=tuple(RAW) + PAIR_FIELDS, pairs=True, flags=0,
             poison=0xAB, **kw):
    """gx_group_pairs itself on host arrays whose every byte is `poison` before the call; returns (rc, totals dict, arrays dict)."""
    p, s = gorp.pair_parts(parts)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    n = len(offsets) - 1
    arrays = {"units": np.zeros(units_cap + 8, data.dtype), "koff": np.zeros(max_keys + 1 + 8, offsets.dtype), "first": np.zeros(max_keys + 8, np.uint32),
              "lines": np.zeros(max_keys + 8, np.uint64), "line_key": np.zeros(n + 8, np.uint32), "pair_units": np.zeros(pair_units_cap + 8, data.dtype),
              "pair_offsets": np.zeros(max_pairs + 1 + 8, offsets.dtype), "pair_key": np.zeros(max_pairs + 8, np.uint32), "pair_first_line": np.zeros(max_pairs + 8, np.uint32),
              "pair_lines": np.zeros(max_pairs + 8, np.uint64), "key_pairs": np.zeros(max_keys + 8, np.uint64), "line_pair": np.zeros(n + 8, np.uint32)}
    for a in arrays.values():
        a.view(np.uint8)[:] = poison
    ptr = lambda name: arrays[name].ctypes.data if name in want else None
    keys = N.gx_group_out(ptr("units"), units_cap, ptr("koff"), ptr("first"), ptr("lines"), None, ptr("line_key"), max_keys)
    out = N.gx_pairs_out(ptr("pair_units"), pair_units_cap, ptr("pair_offsets"), ptr("pair_key"), ptr("pair_first_line"), ptr("pair_lines"), ptr("key_pairs"),
                         ptr("line_pair"), max_pairs)
    totals = N.gx_pairs_totals()
    rc = N.lib().gx_group_pairs(gorp._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, ids.ctypes.data if ids.size else None,
                                None if caps is None or not caps.size else caps.ctypes.data, p.array, p.n, s, None, 0, flags, C.byref(keys),
                                C.byref(out) if pairs else None, C.byref(totals), C.byref(o))
    return rc, Gorp._pairs_totals(totals), arrays


def untouched(arrays, poison=0xAB):
    return all((a.view(np.uint8) == poison).all() for a in arrays.values())


def test_capacities_and_the_size_query(mixed):
    gorp, data, offsets, ids, caps, parts, base = mixed
    t = base["totals"]
    k, ku, p, pu = t["n_keys"], t["key_units"], t["n_pairs"], t["pair_units"]
    exact = dict(max_keys=k, units_cap=ku, max_pairs=p, pair_units_cap=pu)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, **exact)
    assert rc == N.GX_OK and totals == t
    used = {"units": ku, "koff": k + 1, "first": k, "lines": k, "line_key": len(ids), "pair_units": pu, "pair_offsets": p + 1, "pair_key": p, "pair_first_line": p,
            "pair_lines": p, "key_pairs": k, "line_pair": len(ids)}
    for name, m in used.items():
        assert np.array_equal(arrays[name][:m], base[RAW.get(name, name)]), name
        assert (arrays[name][m:].view(np.uint8) == 0xAB).all(), name
    # one short: GX_E_LIMIT, every output byte of pairs AND of keys still poison, the totals filled
    for short in (dict(max_pairs=p - 1), dict(pair_units_cap=pu - 1), dict(max_keys=k - 1), dict(units_cap=ku - 1)):
        rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, **dict(exact, **short))
        assert rc == N.GX_E_LIMIT and totals == t and untouched(arrays), short
    # n_keys > max_keys with key_pairs the only per-key output
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, **dict(exact, max_keys=k - 1), want=("key_pairs", "line_pair", "line_key"))
    assert rc == N.GX_E_LIMIT and totals == t and untouched(arrays)
    # max_pairs sizes the per-pair arrays alone: the seconds, the keys' pairs and the lines' pairs need none beyond the table
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, **dict(exact, max_pairs=p - 1), want=("pair_units", "key_pairs", "line_pair"))
    assert rc == N.GX_OK and np.array_equal(arrays["pair_units"][:pu], base["pair_units"]) and np.array_equal(arrays["key_pairs"][:k], base["key_pairs"])
    # the size query delivers the same totals and writes nothing; max_keys and max_pairs still size the tables
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, max_keys=k, max_pairs=p, want=())
    assert rc == N.GX_OK and totals == t and untouched(arrays)
    # pairs == NULL: the call is gx_group_lines, the pair totals are zero
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, parts, **exact, pairs=False)
    assert rc == N.GX_OK and all(totals[name] == t[name] for name in ("n_keys", "key_units", "lines", "keyed", "unset", "exact"))
    assert (totals["n_pairs"], totals["pair_units"], totals["paired"], totals["unpaired"], totals["pairs_exact"]) == (0, 0, 0, 0, True)
    assert all(np.array_equal(arrays[name][:used[name]], base[RAW[name]]) for name in RAW) and untouched({name: arrays[name] for name in PAIR_FIELDS})
    # ... and with every second -1 the pair passes find every keyed line unpaired
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, [(0, 0, None), (2, 0, None)], max_keys=k, max_pairs=0, want=())
    assert rc == N.GX_OK and totals["n_pairs"] == 0 and totals["paired"] == 0 and totals["unpaired"] == t["keyed"] and totals["pairs_exact"]


def test_a_full_pair_table_and_a_full_key_table():
    gorp = trivial_handle(1)
    # 65 pairs under 3 keys with max_pairs = 32: 64 slots, a full table
    q = np.arange(65 * 3) % 65
    r = np.arange(128) % 64
    data, offsets, ids, caps = named(q % 3, q)
    base = check(gorp, data, offsets, ids, caps, P0)
    assert base["totals"]["n_pairs"] == 65 and base["totals"]["n_keys"] == 3
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0, max_keys=3, units_cap=64, max_pairs=32, pair_units_cap=1024)
    assert rc == N.GX_E_LIMIT and not totals["pairs_exact"] and totals["n_pairs"] == 65 and totals["exact"] and totals["n_keys"] == 3 and untouched(arrays)
    assert totals["paired"] + totals["unpaired"] == totals["keyed"] == len(q)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0, max_keys=3, max_pairs=32, want=())          # (the size query says so too)
    assert rc == N.GX_E_LIMIT and not totals["pairs_exact"] and totals["n_pairs"] == 65
    # 64 pairs fill the 64 slots to the last one; 33 .. 64 > max_pairs pairs with room in the table: exact sizes, nothing written
    data, offsets, ids, caps = named(r % 3, r)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0, max_keys=3, units_cap=64, max_pairs=32, pair_units_cap=1024)
    assert rc == N.GX_E_LIMIT and totals["pairs_exact"] and totals["n_pairs"] == 64 and untouched(arrays)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0, max_keys=3, units_cap=64, max_pairs=32, pair_units_cap=1024, want=("pair_units", "line_pair", "key_pairs"))
    assert rc == N.GX_OK and totals["n_pairs"] == 64 and sorted(arrays["line_pair"][:128].tolist()) == sorted(list(range(64)) * 2)
    # the Python wrapper asks again with what the call reported
    got = gorp.group_pairs(data, offsets, ids, caps, P0, keys="csr", max_pairs=8, pair_units_cap=4)
    assert got["totals"]["n_pairs"] == 64 and got["key_pairs"].tolist() == [22, 21, 21]
    # the KEY table full: gx_group_lines' report, the pair totals zero
    data, offsets, ids, caps = named(np.arange(200), np.arange(200) % 5)
    rc, totals, arrays = raw_call(gorp, data, offsets, ids, caps, P0, max_keys=16, units_cap=4096, max_pairs=200, pair_units_cap=4096)
    assert rc == N.GX_E_LIMIT and not totals["exact"] and totals["n_keys"] == 65 and totals["pairs_exact"] and totals["n_pairs"] == 0 and untouched(arrays)


def test_no_lines_and_no_parts():
    gorp = trivial_handle(1)
    data, offsets, ids, caps = named(np.arange(5), np.arange(5))
    for args in ((data, offsets, ids, caps, []), (data[:0], offsets[:1], ids[:0], caps[:0], P0)):
        got = check(gorp, *args)
        assert got["totals"]["n_pairs"] == 0 and got["pair_offsets"].tolist() == [0] and got["line_pair"].tolist() == [NONE] * (len(args[1]) - 1)


# ---------------------------------------------------------------------------
# one larger draw against the numpy restatement
# ---------------------------------------------------------------------------
def test_300_000_lines_of_1_000_keys_and_50_seconds():
    gorp = trivial_handle(1)
    n = 300000
    kn, sn, extra = draw(n, 1000, 50, seed=18)
    data, offsets, ids, caps = named_batch(kn, sn, extra)
    line_key, key_lines, line_pair, pair_key, pair_first, pair_lines, key_pairs = np_pairs(kn, sn, 50)
    assert len(key_lines) == 1000 and 45000 < len(pair_key) <= 50000
    got = gorp.group_pairs(data, offsets, ids, caps, P0, keys="csr", max_keys=1024)
    t = got["totals"]
    assert t["n_keys"] == 1000 and t["n_pairs"] == len(pair_key) and t["pair_units"] == len(pair_key) and t["paired"] == int(((kn >= 0) & (sn >= 0)).sum())
    assert t["unpaired"] == int(((kn >= 0) & (sn < 0)).sum()) and t["exact"] and t["pairs_exact"]
    for name, want in (("line_key", line_key), ("lines", key_lines), ("line_pair", line_pair), ("pair_key", pair_key), ("pair_first_line", pair_first),
                       ("pair_lines", pair_lines), ("key_pairs", key_pairs)):
        assert got[name].dtype == want.dtype and np.array_equal(got[name], want), name
    assert np.array_equal(got["pair_units"], (sn[pair_first.astype(np.int64)] & 255).astype(np.uint8)) and np.array_equal(got["pair_offsets"], np.arange(len(pair_key) + 1))


# ---------------------------------------------------------------------------
# the README definition, extracted for real; the text form
# ---------------------------------------------------------------------------
def test_readme_definition_end_to_end():
    gorp = Gorp.construct(W.readme3_definition())
    n = 1500
    t_data, _, cat = W.readme3_lines(n, seed=5)
    data = t_data.numpy().copy()
    offsets = (np.arange(n + 1, dtype=np.uint64) * W.LINE_BYTES).astype(np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(ids, cat.numpy().astype(np.int32))
    got = check(gorp, data, offsets, ids, caps, [(k, "verb", "verb") for k in ("PutRequest", "GetRequest", "OtherRequest")])
    assert got["totals"]["n_pairs"] == got["totals"]["n_keys"] and got["key_pairs"].tolist() == [1] * got["totals"]["n_keys"]
    got = check(gorp, data, offsets, ids, caps, VERB_MSEC)
    assert got["totals"]["n_keys"] < got["totals"]["n_pairs"] < got["totals"]["paired"]
    got = check(gorp, data, offsets, ids, caps, VERB_PATH, where=[("GetRequest", "timeTakenInMsec", ">=", 500)])
    assert got["totals"]["n_pairs"] == got["totals"]["paired"]                    # (random paths: a pair per line)
    listed = gorp.group_pairs(data, offsets, ids, caps, VERB_MSEC)
    f = int(listed["pair_first_line"][0])
    assert listed["pairs"][0] == (0, bytes(data[int(offsets[f]) + caps[f, 4]:int(offsets[f]) + caps[f, 5]])) and len(listed["pairs"]) == listed["totals"]["n_pairs"]


@pytest.mark.parametrize("last_newline", [True, False])
def test_text_form_equals_the_batch_form_of_its_lines(last_newline):
    gorp = Gorp.construct(W.readme3_definition())
    rng = np.random.default_rng(9)
    verbs = ["GET", "PUT", "POST", "HEAD"]
    lines = ["[%d]: %s %dms /p/%d" % (i, verbs[int(rng.integers(0, 4))], int(rng.integers(0, 900)), int(rng.integers(0, 40))) for i in range(700)]
    lines[13] = "nothing here"
    text = ("\n".join(lines) + ("\n" if last_newline else "")).encode()
    raw = np.frombuffer(text, np.uint8)
    offsets, _ = split_lines(raw)
    n = len(offsets) - 1
    assert n == 700
    ids, caps = gorp.extract_batch(raw, offsets, strip_eol=True)
    for parts in (VERB_PATH, VERB_MSEC):
        want = check(gorp, raw, offsets, ids, caps, parts)
        got, counts, n_lines = gorp.text_group_pairs(text, parts, keys="csr")
        assert n_lines == n and counts.sum() == n and got["totals"] == want["totals"] and want["totals"]["n_pairs"] > 100
        for name in KEY_FIELDS + PAIR_FIELDS:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    listed, _, _ = gorp.text_group_pairs(text, VERB_PATH)
    assert listed["pairs"][0] == (0, lines[0].split()[3].encode()) and len(listed["pairs"]) == listed["totals"]["n_pairs"]


# ---------------------------------------------------------------------------
# the same batch from host buffers and from device pointers
# ---------------------------------------------------------------------------
def pair_rooms(b, n, t, unit, off_w):
    """every output of a group_pairs_device / text_group_pairs_device call, sized by the totals of its size query"""
    k, ku, p, pu = t["n_keys"], t["key_units"], t["n_pairs"], t["pair_units"]
    return dict(key_units_ptr=b.room("key_units", ku * unit), key_units_cap=ku, key_offsets_ptr=b.room("key_offsets", (k + 1) * off_w),
                key_first_line_ptr=b.room("first_line", k * 4), key_lines_ptr=b.room("lines", k * 8), line_key_ptr=b.room("line_key", n * 4), max_keys=max(k, 1),
                pair_units_ptr=b.room("pair_units", pu * unit), pair_units_cap=pu, pair_offsets_ptr=b.room("pair_offsets", (p + 1) * off_w),
                pair_key_ptr=b.room("pair_key", p * 4), pair_first_line_ptr=b.room("pair_first_line", p * 4), pair_lines_ptr=b.room("pair_lines", p * 8),
                key_pairs_ptr=b.room("key_pairs", k * 8), line_pair_ptr=b.room("line_pair", n * 4), max_pairs=max(p, 1))


@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_host_buffers_and_device_pointers_leave_the_same_bytes(n, compact, offsets_dtype):
    from twin_buffers import twins
    gorp = trivial_handle(3)
    kn, sn, lengths, ids = [i % 7 for i in range(n)], [i % 3 for i in range(n)], [6 + i % 11 for i in range(n)], [i % 3 for i in range(n)]
    if n > 9:
        kn[5], sn[5], lengths[5] = -1, -1, 0                           # an empty line: neither group set
        kn[9], sn[9], ids[9] = -1, -1, -1                              # an unmatched line
    data, offsets, ids, caps = named(kn, sn, lengths=lengths, ids=ids, offsets_dtype=offsets_dtype)
    if compact:
        ids, caps = pack(ids, caps, np.uint16) if n else np.zeros((0, 5), np.uint16), None
    off_w = np.dtype(offsets_dtype).itemsize
    parts = [(0, 0, 1), (1, 0, 1), (2, 0, 1)]
    opts = dict(offsets64=off_w == 8, compact=compact)

    def size_query(b, device_pointers):
        return gorp.group_pairs_device(b.put(data), b.put(offsets), n, b.put(ids), b.put(caps), parts, max_keys=max(n, 1), max_pairs=max(n, 1),
                                       device_pointers=device_pointers, **opts)
    (rc, t), _ = twins(size_query)
    assert rc == N.GX_OK and t["n_keys"] == min(n, 7) and t["n_pairs"] == min(n, 21) and t["paired"] == (n - 2 if n > 9 else n)

    def call(b, device_pointers):
        return gorp.group_pairs_device(b.put(data), b.put(offsets), n, b.put(ids), b.put(caps), parts, device_pointers=device_pointers,
                                       **pair_rooms(b, n, t, 1, off_w), **opts)
    (rc, totals), rooms = twins(call)
    assert rc == N.GX_OK and totals == t
    assert int(np.frombuffer(rooms["pair_lines"], np.uint64)[:t["n_pairs"]].sum()) == t["paired"]


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
        rc, totals, counts, n_lines = gorp.text_group_pairs_device(b.put(text16), text.size, VERB_PATH, max_keys=max(n, 1), max_pairs=max(n, 1),
                                                                   device_pointers=device_pointers)
        return rc, totals, counts.tolist(), n_lines
    (rc, t, counts, n_lines), _ = twins(size_query)
    assert rc == N.GX_OK and n_lines == n and sum(counts) == n and t["paired"] == (n - 2 if n > 9 else n) and t["n_pairs"] == min(n, 21)

    def call(b, device_pointers):
        rc, totals, counts, n_lines = gorp.text_group_pairs_device(b.put(text16), text.size, VERB_PATH, device_pointers=device_pointers, **pair_rooms(b, n, t, 1, 4))
        return rc, totals, counts.tolist(), n_lines
    (rc, totals, counts2, _), rooms = twins(call)
    assert rc == N.GX_OK and totals == t and counts2 == counts
    assert int(np.frombuffer(rooms["pair_lines"], np.uint64)[:t["n_pairs"]].sum()) == t["paired"]
