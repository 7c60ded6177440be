"""GPU tests of the partition calls: gx_partition_lines, gx_text_to_jsonl_by_extraction.

Expected values are a numpy restatement written here: the outcome index of every id, key = the outcome where it is wanted,
else 2K + 1, a STABLE argsort of the keys cut at the number of kept lines, then slices of the input, np.cumsum of the permuted
lengths and np.bincount of the keys.  Ids are synthetic wherever the test is about the partition (it takes any id column, as
the selection does).  Everything is compared exactly."""
import ctypes as C
import json
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 2048    # gx_scan.hpp: items per workgroup of the scan
SORT_BLOCK = 2048    # gx_partition.hip: PART_BLOCK, the lines one workgroup of the sort's count and scatter passes owns
DIGIT_BITS = 6       # gx_partition.hip: a digit of the radix sort; keys are 0 .. 2K + 1


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def outcome(ids, K):
    v = np.asarray(ids, dtype=np.int64)
    oc = np.full(v.shape, 2 * K + 1, np.int64)
    oc = np.where((v >= 0) & (v < K), v, oc)
    oc = np.where(v == -1, K, oc)
    return np.where((v <= -2) & (v >= -1 - K), K + 1 + (-2 - v), oc)


def restate(data, offsets, ids, mask, K):
    """(index, units, offsets, group_lines, group_units) of the partition `mask` (uint8[2K + 1] or None) over a CSR batch."""
    oc = outcome(ids, K)
    want = np.ones(2 * K + 1, np.uint8) if mask is None else np.asarray(mask, np.uint8)
    key = np.where(np.append(want, 0)[oc] != 0, oc, 2 * K + 1)
    kept = int(np.count_nonzero(key <= 2 * K))
    order = np.argsort(key, kind="stable")[:kept]
    off = np.asarray(offsets).astype(np.int64)
    lens = (off[1:] - off[:-1])[order]
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    units = data[np.repeat(off[:-1][order] - out_off[:-1], lens) + np.arange(out_off[-1])] if kept else data[:0]
    per_group = np.bincount(key, minlength=2 * K + 2)[:2 * K + 1]
    group_lines = np.concatenate([[0], np.cumsum(per_group), [kept]]).astype(np.uint64)       # [2K + 3]; bin 2K + 1 is an empty group
    group_units = out_off[group_lines.astype(np.int64)].astype(np.uint64)
    return order.astype(np.uint32), units, out_off.astype(offsets.dtype), group_lines, group_units


def id_column(ids):
    return ids if ids.ndim == 1 else ids[:, 0].astype({2: np.int16, 1: np.int8}[ids.itemsize])


def check_partition(gorp, data, offsets, ids, mask, caps=None):
    K = gorp.num_extractions
    index, units, out_off, group_lines, group_units = restate(data, offsets, id_column(ids), mask, K)
    got = gorp.partition_lines(data, offsets, ids, rows=caps, want=mask)
    assert np.array_equal(got[0], index)
    assert got[1].dtype == data.dtype and np.array_equal(got[1], units)
    assert got[2].dtype == offsets.dtype and np.array_equal(got[2], out_off)
    assert np.array_equal(got[-2], group_lines) and np.array_equal(got[-1], group_units)
    assert np.array_equal(got[3], ids[index]) if len(got) > 5 else caps is None and ids.ndim == 1
    if caps is not None:
        assert np.array_equal(got[4], caps[index])
    return got


def oracle_for(definition):
    built = [e.build() for e in definition]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


def pack_rows(ids, caps, dtype):
    """Result rows in the u16 / u8 format (gx_layout.hpp) from dense ids and offsets that all fit."""
    rows = np.concatenate([np.asarray(ids, np.int64)[:, None], np.asarray(caps, np.int64)], axis=1)
    assert rows.max() < np.iinfo(dtype).max - 1
    return (rows & np.iinfo(dtype).max).astype(dtype)


# the definition and the lines of test_gpu_select.py, restated: all three kinds of outcome
THREE = [FlattenedExtraction("ab", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),   # "a\rb": the automaton says yes, the regexp no
         FlattenedExtraction("cee", [["text", "c"], ["extractor", "w", [["pattern", "\\w*"]]]]),
         FlattenedExtraction("dee", [["text", "d="], ["extractor", "n", [["pattern", "\\d+"]]], ["pattern", ".*"]])]
K3 = 3


def three_outcome_lines(n, seed, max_len=700):
    rng = random.Random(seed)
    lines = []
    for _ in range(n):
        kind = rng.random()
        length = rng.choice([0, 1, 2, 15, 16, 17]) if rng.random() < 0.1 else rng.randrange(0, max_len + 1)
        body = bytes(rng.choice(b"abcd xyz019=\t") for _ in range(max(0, length - 2)))
        if kind < 0.25:
            ln = b"a" + body + b"b"
        elif kind < 0.35:
            ln = b"a" + body[:len(body) // 2] + b"\r" + body[len(body) // 2:] + b"b"
        elif kind < 0.5:
            ln = b"c" + bytes(rng.choice(b"abc_019") for _ in range(max(0, length - 1)))
        elif kind < 0.65:
            ln = b"d=" + b"7" * rng.randrange(1, 6) + body
        elif kind < 0.75:
            ln = b""
        else:
            ln = body
        lines.append(ln[:max_len])
    return lines


@pytest.fixture(scope="module")
def three():
    return Gorp.construct(THREE), oracle_for(THREE)


@pytest.fixture(scope="module")
def three_batch(three):
    """5 000 lines with every kind of outcome, and the oracle's rows for them (computed once, never changed)."""
    lines = three_outcome_lines(5000, seed=11)
    data, offsets = lines_to_csr(lines)
    ids, caps = three[1].extract_batch(data, offsets)
    for a in (data, offsets, ids, caps):
        a.setflags(write=False)
    return data, offsets, ids, caps


# ---------------------------------------------------------------------------
# 1. every kind of outcome
# ---------------------------------------------------------------------------
def test_every_kind_of_outcome_and_eight_masks(three, three_batch):
    gorp = three[0]
    data, offsets, ids, caps = three_batch
    counts = np.bincount(outcome(ids, K3), minlength=2 * K3 + 2)
    assert (counts[:K3 + 2] > 0).all() and counts[2 * K3 + 1] == 0      # three extractions, unmatched, exceptions of "ab"
    got = check_partition(gorp, data, offsets, ids, None, caps=caps)
    assert len(got[0]) == len(ids) and np.array_equal(np.diff(got[-2].astype(np.int64))[:2 * K3 + 1], counts[:2 * K3 + 1])
    masks = [[0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0],
             [0, 1, 0, 1, 0, 1, 0], [1, 0, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1]]
    for mask in masks:
        check_partition(gorp, data, offsets, ids, np.array(mask, np.uint8), caps=caps)
    assert np.array_equal(check_partition(gorp, data, offsets, ids, np.ones(7, np.uint8))[0], got[0])   # want=None is "all of 0 .. 2K"


# ---------------------------------------------------------------------------
# 2. line counts around the tile, the scan block and the sort workgroup
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted({0, 1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1,
                                      3 * SORT_BLOCK + 17}))
def test_line_counts_around_tile_scan_and_sort_boundaries(three, n):
    gorp = three[0]
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 40, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = rng.integers(1, 255, int(offsets[-1]), dtype=np.uint8)
    ids = rng.choice(np.array([0, 1, 2, -1, -2, -3, -4], np.int32), n)
    for want in (None, "unmatched", [0, 2, "exceptions"]):
        check_partition(gorp, data, offsets, ids, None if want is None else gorp.want_mask(want))


# ---------------------------------------------------------------------------
# 3. digit boundaries: 2K + 2 keys take one digit up to K = 31, two up to K = 2047, three beyond
# ---------------------------------------------------------------------------
def digits_of(K):
    return -(-int(2 * K + 1).bit_length() // DIGIT_BITS)


_literal_handles = {}


def literal_handle(K):
    if K not in _literal_handles:
        _literal_handles[K] = Gorp.construct([FlattenedExtraction("k%04d" % k, [["text", "k%04d=" % k], ["extractor", "v", [["pattern", "\\d+"]]]])
                                              for k in range(K)])
    return _literal_handles[K]


@pytest.mark.parametrize("K", [1, 31, 32, 2047, 2048])
def test_digit_boundaries(K):
    assert [digits_of(k) for k in (1, 31, 32, 2047, 2048)] == [1, 1, 2, 2, 3]
    gorp = literal_handle(K)
    assert gorp.num_extractions == K
    n = 20000
    rng = np.random.default_rng(K)
    lens = rng.integers(0, 24, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = rng.integers(1, 255, int(offsets[-1]), dtype=np.uint8)
    top = 2 * K          # the largest outcome that can be kept: the exception of extraction K - 1

    def ids_of(oc):
        oc = np.asarray(oc, np.int64)
        return np.where(oc < K, oc, np.where(oc == K, -1, -2 - (oc - K - 1))).astype(np.int32)

    descending = np.arange(n) % (top + 1)
    descending = (top - descending)                       # every outcome once, descending, again and again
    patterns = {
        "all one outcome": np.full(n, top // 2),
        "every outcome, descending": descending,
        "alternating, two high digits": np.where(np.arange(n) % 2 == 0, top, 0),       # top and 0 differ in the last digit
        "uniform": rng.integers(0, top + 1, n),
    }
    for name, oc in patterns.items():
        ids = ids_of(oc)
        assert np.array_equal(outcome(ids, K), oc), name
        check_partition(gorp, data, offsets, ids, None)
    # ids outside the range: bin 2K + 1, counted out, never written
    ids = ids_of(patterns["uniform"])
    hit = rng.random(n) < 0.05
    ids[hit] = rng.choice(np.array([K, K + 12345, -2 - K, -2 ** 31, 2 ** 31 - 1], np.int64), int(hit.sum())).astype(np.int32)
    got = check_partition(gorp, data, offsets, ids, None)
    assert len(got[0]) == n - hit.sum() and not hit[got[0]].any() and got[-2][2 * K + 1] == got[-2][2 * K + 2] == n - hit.sum()
    mask = (rng.random(2 * K + 1) < 0.5).astype(np.uint8)
    check_partition(gorp, data, offsets, ids, mask)


# ---------------------------------------------------------------------------
# 4. alignment: every source misalignment, every line length 0..80, destinations fenced by poison
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mis", range(16))
def test_alignment_sweep_with_poisoned_destination(three, mis):
    import torch
    gorp = three[0]
    rng = np.random.default_rng(5 + mis)
    lens = np.concatenate([rng.permutation(81), rng.permutation(81)])          # every length 0..80, twice, in some order
    n = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(offsets[-1])
    payload = rng.integers(1, 255, total, dtype=np.uint8)
    ids = rng.choice(np.array([0, 1, 2, -1, -2], np.int32), n)                  # five outcomes
    ids[-1] = -2                                                                # (the batch's last line is the output's last: both end at their buffer's end)
    d_off = torch.from_numpy(offsets.view(np.int32)).cuda()
    d_ids = torch.from_numpy(ids).cuda()
    POISON, FENCE = 0xA5, 64
    src_buf = torch.empty(mis + total, dtype=torch.uint8, device="cuda")        # sized exactly: the batch ends where the tensor ends
    src_buf[mis:] = torch.from_numpy(payload).cuda()
    for mask in (None, np.array([1, 0, 1, 0, 1, 0, 0], np.uint8), np.array([0, 1, 0, 1, 0, 0, 0], np.uint8)):
        index, units, out_off, group_lines, group_units = restate(payload, offsets, ids, mask, K3)
        for dst_mis in (0, 3, 8, 13):
            dst = torch.full((FENCE + dst_mis + len(units) + FENCE,), POISON, dtype=torch.uint8, device="cuda")
            exact = torch.full((len(units),), POISON, dtype=torch.uint8, device="cuda")   # the last line ends at the buffer's end
            d_index = torch.full((len(index) + 2,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
            d_ooff = torch.full((len(index) + 3,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
            where = (mis, dst_mis, None if mask is None else mask.tolist())
            for target, at in ((dst, FENCE + dst_mis), (exact, 0)):
                got = gorp.partition_lines_device(src_buf.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), None, mask,
                                                  out_index_ptr=d_index.data_ptr() + 4, out_data_ptr=target.data_ptr() + at,
                                                  out_offsets_ptr=d_ooff.data_ptr() + 4, cap_lines=len(index), out_bytes_cap=len(units))
                assert got[:2] == (len(index), len(units)), where
                assert np.array_equal(got[2], group_lines) and np.array_equal(got[3], group_units), where
            out = dst.cpu().numpy()
            assert (out[:FENCE + dst_mis] == POISON).all() and (out[FENCE + dst_mis + len(units):] == POISON).all(), where
            assert np.array_equal(out[FENCE + dst_mis:FENCE + dst_mis + len(units)], units), where
            assert np.array_equal(exact.cpu().numpy(), units), where
            oi, oo = d_index.cpu().numpy(), d_ooff.cpu().numpy()
            assert oi[0] == oi[-1] == 0x7FFFFFFF and np.array_equal(oi[1:-1].view(np.uint32), index), where
            assert oo[0] == oo[-1] == 0x7FFFFFFF and np.array_equal(oo[1:-1].view(np.uint32), out_off), where


# ---------------------------------------------------------------------------
# 5. formats
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_id_formats_and_offset_widths(three, fmt, offsets_dtype):
    gorp, orc = three
    lines = three_outcome_lines(3000, seed=23, max_len=250)                     # (u8 rows: offsets below 255)
    data, offsets = lines_to_csr(lines, offsets_dtype=offsets_dtype)
    ids, caps = orc.extract_batch(data, offsets)
    for want in (None, "exceptions", ["ab", "dee"], ["cee", "unmatched", "exceptions"]):
        mask = None if want is None else gorp.want_mask(want)
        if fmt == "int32":
            check_partition(gorp, data, offsets, ids, mask, caps=caps)
            check_partition(gorp, data, offsets, ids, mask)
        else:
            check_partition(gorp, data, offsets, pack_rows(ids, caps, np.uint16 if fmt == "u16" else np.uint8), mask)


def test_utf16_batch_with_units_above_0xff(three):
    gorp, orc = three
    rng = random.Random(3)
    alphabet = "abcd =019Ж€中\r"
    lines = []
    for _ in range(2000):
        body = "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 120)))
        lines.append(rng.choice(["a%sb", "c%s", "d=1%s", "%s", "a€%sb"]) % body)
    units = [np.frombuffer(s.encode("utf-16-le"), dtype=np.uint16) for s in lines]
    data = np.concatenate(units)
    offsets = np.concatenate([[0], np.cumsum([len(u) for u in units])]).astype(np.uint32)
    assert (data > 0xFF).any()
    ids = np.array([orc.extract(s)[0] for s in lines], np.int32)
    assert len(set(outcome(ids, K3).tolist())) >= 4
    for want in (None, "exceptions", ["cee", "dee", "unmatched"]):
        check_partition(gorp, data, offsets, ids, None if want is None else gorp.want_mask(want))


def test_lines_keep_their_terminators(three):
    gorp, orc = three
    rng = random.Random(9)
    text = b"".join(ln.replace(b"\r", b"") + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in three_outcome_lines(1500, seed=4, max_len=120)) + b"a last line without one b"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    _, ref_lines, _ = O.read_lines(text)
    ids = np.array([orc.extract(ln)[0] for ln in ref_lines], np.int32)
    for want in (None, ["ab", "cee"], "unmatched"):
        got = check_partition(gorp, data, offsets, ids, None if want is None else gorp.want_mask(want))
        assert got[1].tobytes() == b"".join(text[offsets[i]:offsets[i + 1]] for i in got[0])
    got = check_partition(gorp, data, offsets, ids, None)
    assert sorted(got[0].tolist()) == list(range(len(ids)))
    # the unterminated line matches "ab", outcome 0: it closes group 0 and still ends where the text ended, with no terminator added
    last = int(got[-2][1]) - 1
    assert ids[-1] == 0 and got[0][last] == len(ids) - 1 and got[2][last + 1] == got[-1][1]
    assert got[1][got[2][last]:got[2][last + 1]].tobytes() == b"a last line without one b"


# ---------------------------------------------------------------------------
# 6. capacities
# ---------------------------------------------------------------------------
def test_capacity_too_small_writes_nothing_and_size_query_equals_run(three, three_batch):
    import torch
    gorp = three[0]
    data, offsets, ids, caps = three_batch
    mask = gorp.want_mask(["ab", "dee", "exceptions"])
    index, units, out_off, group_lines, group_units = restate(data, offsets, ids, mask, K3)
    k, nbytes = len(index), len(units)
    d = {name: torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).cuda() for name, a in
         (("data", data), ("off", offsets), ("ids", ids), ("caps", caps))}
    inputs = (d["data"].data_ptr(), d["off"].data_ptr(), len(ids), d["ids"].data_ptr(), d["caps"].data_ptr(), mask)
    query = gorp.partition_lines_device(*inputs)                               # the size query
    assert query[:2] == (k, nbytes) and np.array_equal(query[2], group_lines) and np.array_equal(query[3], group_units)
    POISON = 0x5A
    sizes_of = {"out_index_ptr": 4 * k, "out_data_ptr": nbytes, "out_offsets_ptr": 4 * (k + 1), "out_ids_ptr": 4 * k, "out_caps_ptr": 4 * k * caps.shape[1]}
    outs = {name: torch.full((size,), POISON, dtype=torch.uint8, device="cuda") for name, size in sizes_of.items()}
    ptrs = {name: t.data_ptr() for name, t in outs.items()}
    L = N.lib()
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    for cap_lines, cap_bytes in ((k - 1, nbytes), (k, nbytes - 1), (0, 0)):
        sizes = (C.c_uint64(0), C.c_uint64(0))
        gl, gu = np.zeros(2 * K3 + 3, np.uint64), np.zeros(2 * K3 + 3, np.uint64)
        rc = L.gx_partition_lines(gorp._h.ptr, *inputs[:5], mask.ctypes.data, ptrs["out_index_ptr"], ptrs["out_data_ptr"], ptrs["out_offsets_ptr"],
                                  ptrs["out_ids_ptr"], ptrs["out_caps_ptr"], cap_lines, cap_bytes, gl.ctypes.data, gu.ctypes.data,
                                  C.byref(sizes[0]), C.byref(sizes[1]), C.byref(o))
        assert rc == N.GX_E_LIMIT and "smaller than" in N.last_error()
        assert (sizes[0].value, sizes[1].value) == (k, nbytes) and np.array_equal(gl, group_lines) and np.array_equal(gu, group_units)
        for t in outs.values():
            assert bool((t == POISON).all())
    with pytest.raises(GorpError) as ei:
        gorp.partition_lines_device(*inputs, cap_lines=k - 1, out_bytes_cap=nbytes, **ptrs)
    assert ei.value.code == N.GX_E_LIMIT
    assert gorp.partition_lines_device(*inputs, cap_lines=k, out_bytes_cap=nbytes, **ptrs)[:2] == (k, nbytes)
    assert np.array_equal(outs["out_data_ptr"].cpu().numpy(), units)
    assert np.array_equal(outs["out_index_ptr"].cpu().numpy().view(np.uint32), index)
    assert np.array_equal(outs["out_offsets_ptr"].cpu().numpy().view(np.uint32), out_off)
    assert np.array_equal(outs["out_ids_ptr"].cpu().numpy().view(np.int32), ids[index])
    assert np.array_equal(outs["out_caps_ptr"].cpu().numpy().view(np.int32).reshape(k, -1), caps[index])


# ---------------------------------------------------------------------------
# 7. stream order
# ---------------------------------------------------------------------------
def test_partition_follows_a_no_sync_batch_on_its_stream():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L, K = 300000, 200, 3
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.full((n, width), 0x55, dtype=torch.uint8, device="cuda")       # ids nobody wrote: outcome 2K + 1
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    inputs = (data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, None)
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True,
                                  compact=2, line_bytes_hint=L)
        k, nbytes, group_lines, _ = gorp.partition_lines_device(*inputs, compact=2, stream=stream.cuda_stream)
        index = torch.empty(k, dtype=torch.int32, device="cuda")
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gorp.partition_lines_device(*inputs, out_index_ptr=index.data_ptr(), out_data_ptr=out.data_ptr(), cap_lines=k, out_bytes_cap=nbytes,
                                    compact=2, stream=stream.cuda_stream)
        index2 = torch.empty(k, dtype=torch.int32, device="cuda")
        out2 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gorp.partition_lines_device(*inputs, out_index_ptr=index2.data_ptr(), out_data_ptr=out2.data_ptr(), cap_lines=k, out_bytes_cap=nbytes,
                                    compact=2, stream=stream.cuda_stream, no_sync=True)
    # the copy pass of that last call may still be reading the handle's workspace: a call on ANOTHER stream waits for it before it
    # lays out its own, and neither result suffers
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        counts = gorp.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=other.cuda_stream)
    stream.synchronize()
    oc = torch.where(cat >= 0, cat.long(), torch.full_like(cat, K).long())
    order = torch.sort(oc, stable=True).indices
    assert k == n and nbytes == n * L and counts[2 * K + 1] == 0               # the partition saw the rows the extraction wrote
    assert np.array_equal(group_lines[:2 * K + 2], np.concatenate([[0], np.cumsum(counts[:2 * K + 1])]).astype(np.uint64))
    assert torch.equal(index, order.to(torch.int32)) and torch.equal(index2, index)
    assert torch.equal(out, data.view(n, L)[order].reshape(-1)) and torch.equal(out2, out)


# ---------------------------------------------------------------------------
# 8. determinism
# ---------------------------------------------------------------------------
def test_two_runs_over_200k_lines_are_bit_identical(three):
    import torch
    gorp = three[0]
    n = 200000
    rng = np.random.default_rng(88)
    lens = rng.integers(0, 60, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(offsets[-1])
    d_data = torch.from_numpy(rng.integers(1, 255, total, dtype=np.uint8)).cuda()
    d_off = torch.from_numpy(offsets.view(np.int32)).cuda()
    d_ids = torch.from_numpy(rng.choice(np.array([0, 1, 2, -1, -2, -3, -4, 9], np.int32), n)).cuda()
    runs = []
    for _ in range(2):
        outs = [torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(total, dtype=torch.uint8, device="cuda"),
                torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")]
        got = gorp.partition_lines_device(d_data.data_ptr(), d_off.data_ptr(), n, d_ids.data_ptr(), None, None, out_index_ptr=outs[0].data_ptr(),
                                          out_data_ptr=outs[1].data_ptr(), out_offsets_ptr=outs[2].data_ptr(), out_ids_ptr=outs[3].data_ptr(),
                                          cap_lines=n, out_bytes_cap=total)
        runs.append((got, outs))
    (a, outs_a), (b, outs_b) = runs
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and 0 < a[0] < n
    for x, y in zip(outs_a, outs_b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------
# 9. composition
# ---------------------------------------------------------------------------
def test_partitioned_batch_composes_with_extract_jsonl_and_select(three, three_batch):
    gorp, orc = three
    data, offsets, ids, caps = three_batch
    index, pdata, poff, pids, pcaps, group_lines, group_units = check_partition(gorp, data, offsets, ids, None, caps=caps)
    again_ids, again_caps = gorp.extract_batch(pdata, poff)
    assert np.array_equal(again_ids, pids) and np.array_equal(again_caps, pcaps)
    # JSON Lines over the partitioned batch = the per-group concatenation of the oracle's lines
    lines = [bytes(data[offsets[i]:offsets[i + 1]]) for i in range(len(ids))]
    xs = gorp.getExtractions()
    whole, woff = O.results_to_jsonl(lines, ids, caps, [x.getName() for x in xs], [x._extractorNames for x in xs], [x.getExtra() for x in xs], id_as="id")
    want_text = b"".join(whole[int(woff[i]):int(woff[i + 1])] for k in range(K3) for i in np.flatnonzero(ids == k))
    assert len(want_text) > 0 and gorp.results_to_jsonl(pdata, poff, pids, pcaps, id_as="id") == want_text
    # gx_select_lines(want = x) is group x
    for x in range(2 * K3 + 1):
        mask = np.zeros(2 * K3 + 1, np.uint8)
        mask[x] = 1
        sel = gorp.select_lines(data, offsets, ids, rows=caps, want=mask)
        lo, hi = int(group_lines[x]), int(group_lines[x + 1])
        assert np.array_equal(sel[0], index[lo:hi])
        assert np.array_equal(sel[1], pdata[int(group_units[x]):int(group_units[x + 1])])
        assert np.array_equal(sel[2].astype(np.int64), poff[lo:hi + 1].astype(np.int64) - int(poff[lo]))
        assert np.array_equal(sel[3], pids[lo:hi]) and np.array_equal(sel[4], pcaps[lo:hi])


# ---------------------------------------------------------------------------
# 10. 64 real rules: two digits, uneven lines, ids from the library's own extraction
# ---------------------------------------------------------------------------
def test_syslog_200k_uneven_lines_64_rules():
    definition, meta = W.syslog_definition(64)
    gorp = Gorp.construct(definition)
    data, offsets, _ = W.syslog_lines(meta, 200000, seed=8, min_len=50, max_len=2000)
    ids, caps = gorp.extract_batch(data, offsets)
    assert digits_of(64) == 2 and len(set(outcome(ids, 64).tolist())) > 64
    check_partition(gorp, data, offsets, ids, None, caps=caps)
    check_partition(gorp, data, offsets, ids, gorp.want_mask(list(range(0, 64, 2)) + ["unmatched"]))


# ---------------------------------------------------------------------------
# 11. two million lines on the device, u8 rows
# ---------------------------------------------------------------------------
def test_two_million_lines_on_the_device():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    K, n, L = 3, 2 * 1000 * 1000, 200
    data, offsets, cat = W.readme3_lines(n, seed=12, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)                              # (below 2^31: the same bits as uint32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), compact=2, line_bytes_hint=L)
    ids = rows[:, 0].view(torch.int8).to(torch.int64)
    assert torch.equal(ids, cat.to(torch.int64))
    oc = torch.where(ids >= 0, ids, torch.where(ids == -1, K, K + 1 + (-2 - ids)))
    for want in (None, ["PutRequest", "OtherRequest", "unmatched"]):
        mask = None if want is None else gorp.want_mask(want)
        wanted = torch.ones(2 * K + 2, dtype=torch.bool, device="cuda") if mask is None else torch.from_numpy(np.append(mask, 0).astype(bool)).cuda()
        wanted[2 * K + 1] = False
        key = torch.where(wanted[oc], oc, torch.full_like(oc, 2 * K + 1))
        sorted_key, order = torch.sort(key, stable=True)
        k = int((sorted_key <= 2 * K).sum())
        order = order[:k]
        got = gorp.partition_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, mask, compact=2)
        assert got[:2] == (k, k * L)
        out = torch.empty(k * L, dtype=torch.uint8, device="cuda")
        o_index = torch.empty(k, dtype=torch.int32, device="cuda")
        o_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        o_rows = torch.empty((k, width), dtype=torch.uint8, device="cuda")
        got = gorp.partition_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, mask, out_index_ptr=o_index.data_ptr(),
                                          out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_rows.data_ptr(),
                                          cap_lines=k, out_bytes_cap=k * L, compact=2)
        assert torch.equal(o_index, order.to(torch.int32))
        assert torch.equal(out, data.view(n, L).index_select(0, order).reshape(-1))
        assert torch.equal(o_off, (torch.arange(k + 1, device="cuda") * L).to(torch.int32))
        assert torch.equal(o_rows, rows.index_select(0, order))
        per_group = torch.bincount(key, minlength=2 * K + 2)[:2 * K + 1].cumsum(0).cpu().numpy()
        group_lines = np.concatenate([[0], per_group, [k]]).astype(np.uint64)
        assert np.array_equal(got[2], group_lines) and np.array_equal(got[3], group_lines * np.uint64(L))


# ---------------------------------------------------------------------------
# 12. whole files: gx_text_to_jsonl_by_extraction
# ---------------------------------------------------------------------------
def regrouped(jsonl, names):
    """The lines of a JSON Lines text grouped stably by their "rule" value, in the order of `names`; and where every group begins."""
    lines = jsonl.splitlines(keepends=True)
    rule_of = [json.loads(ln.decode("utf-8"))["rule"] for ln in lines]
    groups = [b"".join(ln for ln, r in zip(lines, rule_of) if r == name) for name in names]
    return b"".join(groups), np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)


def check_by_extraction(gorp, text, names, utf8=False):
    K = len(names)
    jsonl, n_lines, n_matched, _ = gorp.text_to_jsonl(text, id_as="rule", utf8=utf8)
    want_text, want_groups = regrouped(jsonl, names)
    got, group_out, counts, n_lines2 = gorp.text_to_jsonl_by_extraction(text, id_as="rule", utf8=utf8)
    assert got == want_text and np.array_equal(group_out, want_groups) and n_lines2 == n_lines
    assert np.array_equal(counts, gorp.text_select(text, "unmatched", utf8=utf8)[1]) and counts[:K].sum() == n_matched
    raw = np.frombuffer(text, dtype=np.uint8)
    query = gorp.text_to_jsonl_by_extraction_device(raw.ctypes.data if raw.size else None, raw.size, None, 0, id_as="rule", utf8=utf8,
                                                    device_pointers=False)
    assert query[0] == len(got) and np.array_equal(query[1], group_out) and np.array_equal(query[2], counts) and query[3] == n_lines
    return got, group_out, counts


def test_text_to_jsonl_by_extraction_on_the_readme_definition():
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    data, offsets, cat = W.readme3_lines(20000, seed=61)
    d, o = data.numpy(), offsets.numpy().astype(np.int64)
    rng = random.Random(6)
    text = b"".join(bytes(d[o[i]:o[i + 1]]) + rng.choice([b"\n", b"\n", b"\r\n"]) for i in range(len(o) - 1)) + b"[123456789]: GET 5ms /tail"
    got, group_out, counts = check_by_extraction(gorp, text, ["PutRequest", "GetRequest", "OtherRequest"])
    assert (np.diff(group_out.astype(np.int64)) > 0).all() and got.endswith(b"\n")
    assert check_by_extraction(gorp, b"", ["PutRequest", "GetRequest", "OtherRequest"])[0] == b""
    with pytest.raises(GorpError) as ei:
        raw = np.frombuffer(text, dtype=np.uint8)
        out = np.zeros(len(got), np.uint8)
        gorp.text_to_jsonl_by_extraction_device(raw.ctypes.data, raw.size, out.ctypes.data, len(got) - 1, id_as="rule", device_pointers=False)
    assert ei.value.code == N.GX_E_LIMIT


def test_text_to_jsonl_by_extraction_on_three_outcome_kinds(three):
    gorp = three[0]
    rng = random.Random(19)
    body = [ln.replace(b"\r", b"").replace(b"\t", b" ") for ln in three_outcome_lines(4000, seed=14, max_len=150)]
    text = b"".join(ln + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in body) + b"\n\n" + b"a last line without one b"
    got, group_out, counts = check_by_extraction(gorp, text, ["ab", "cee", "dee"])
    assert (counts[:K3 + 1] > 0).all() and (np.diff(group_out.astype(np.int64)) > 0).all()


def test_text_to_jsonl_by_extraction_utf8(three):
    gorp = three[0]
    rng = random.Random(29)
    lines = []
    for _ in range(3000):
        body = "".join(rng.choice("abcd =019" + ("中é" if rng.random() < 0.3 else "")) for _ in range(rng.randrange(0, 60)))
        lines.append(rng.choice(["a%sb", "c%s", "d=1%s", "%s"]) % body)
    text = "\n".join(lines).encode("utf-8") + b"\n"
    assert "中".encode("utf-8") in text and "é".encode("utf-8") in text
    got, group_out, counts = check_by_extraction(gorp, text, ["ab", "cee", "dee"], utf8=True)
    assert "中".encode("utf-8") in got and (np.diff(group_out.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_text_to_jsonl_by_extraction_from_host_buffers_and_device_pointers(n):
    """the same text once from a host buffer and once from a device pointer: equal sizes, groups, counts, line count and bytes; every
    matched line's object lies in its extraction's group (among 65 lines one is empty and one matches nothing)"""
    from twin_buffers import twins
    gorp = Gorp.construct(W.readme3_definition())
    lines = ["[%d]: %s %dms /p/%d" % (i, ("GET", "PUT", "POST")[i % 3], 10 * i, i % 7) for i in range(n)]
    if n > 9:
        lines[5], lines[9] = "", "nothing here"
    text = np.frombuffer("".join(l + "\n" for l in lines).encode(), np.uint8)
    text16 = np.zeros((text.size + 15) // 16 * 16 + 16, np.uint8)       # (a device text is 16-byte aligned: torch's allocations are)
    text16[:text.size] = text

    def size_query(b, device_pointers):
        size, group_out, counts, n_lines = gorp.text_to_jsonl_by_extraction_device(b.put(text16), text.size, None, 0, id_as="rule", device_pointers=device_pointers)
        return size, group_out.tolist(), counts.tolist(), n_lines
    (size, group_out, counts, n_lines), _ = twins(size_query)
    matched = n - 2 if n > 9 else n
    assert n_lines == n and sum(counts) == n and sum(counts[:3]) == matched and group_out[0] == 0 and group_out[-1] == size

    def call(b, device_pointers):
        got, g, c, nl = gorp.text_to_jsonl_by_extraction_device(b.put(text16), text.size, b.room("out", size), size, id_as="rule", device_pointers=device_pointers)
        return got, g.tolist(), c.tolist(), nl
    (got, group_out2, counts2, _), rooms = twins(call)
    assert got == size and group_out2 == group_out and counts2 == counts
    objects = rooms["out"][:size].split(b"\n")[:-1] if size else []
    assert len(objects) == matched
    for k in range(3):
        part = rooms["out"][group_out[k]:group_out[k + 1]]
        assert part.count(b"\n") == counts[k] and all(b'"rule"' in o for o in part.split(b"\n")[:-1])
