"""GPU tests of the outcome calls: gx_count_outcomes, gx_select_lines, gx_text_select.

Expected values are a numpy restatement written here -- np.flatnonzero of the mask, np.cumsum of the kept lengths, slices of
the input, np.bincount of the outcome index -- applied to the ids that OracleGorp.extract_batch gives for the same lines (the
large device-resident batch: torch masked ops on the generator's own categories).  Everything is compared exactly."""
import ctypes as C
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 2048              # gx_scan.hpp: items per workgroup of the scan
SCAN_CHUNK = 1024 * SCAN_BLOCK   # ... and per round of its one-workgroup pass over the block sums


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
    """(index, units, offsets, counts) of the selection `mask` (uint8[2K + 1]) over a CSR batch."""
    oc = outcome(ids, K)
    keep = np.append(np.asarray(mask, np.uint8), 0)[oc] != 0          # (bin 2K + 1 is never selected)
    index = np.flatnonzero(keep).astype(np.uint32)
    off = np.asarray(offsets).astype(np.int64)
    lens = off[1:] - off[:-1]
    out_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(offsets.dtype)
    units = data[off[0]:off[-1]][np.repeat(keep, lens)]
    counts = np.bincount(oc, minlength=2 * K + 2).astype(np.uint64)
    return index, units, out_off, counts


def oracle_for(definition):
    built = [e.build() for e in definition]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


def pack_rows(ids, caps, dtype):
    """Result rows in the u16 / u8 format (gx_layout.hpp) from dense ids and offsets that all fit."""
    rows = np.concatenate([np.asarray(ids, np.int64)[:, None], np.asarray(caps, np.int64)], axis=1)
    assert rows.max() < np.iinfo(dtype).max - 1
    return (rows & np.iinfo(dtype).max).astype(dtype)


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


def check_selection(gorp, data, offsets, ids, mask, caps=None):
    K = gorp.num_extractions
    index, units, out_off, _ = restate(data, offsets, ids if ids.ndim == 1 else ids[:, 0].astype({2: np.int16, 1: np.int8}[ids.itemsize]), mask, K)
    got = gorp.select_lines(data, offsets, ids, rows=caps, want=mask)
    assert np.array_equal(got[0], index)
    assert got[1].dtype == data.dtype and np.array_equal(got[1], units)
    assert got[2].dtype == offsets.dtype and np.array_equal(got[2], out_off)
    assert np.array_equal(got[3], ids[index]) if len(got) > 3 else caps is None and ids.ndim == 1
    if caps is not None:
        assert np.array_equal(got[4], caps[index])
    return got


# ---------------------------------------------------------------------------
# every mask over a definition with all three kinds of outcome
# ---------------------------------------------------------------------------
def test_every_mask_over_three_outcome_kinds():
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    lines = three_outcome_lines(5000, seed=11)
    data, offsets = lines_to_csr(lines)
    ids, caps = orc.extract_batch(data, offsets)
    gids, gcaps = gorp.extract_batch(data, offsets)
    assert np.array_equal(gids, ids) and np.array_equal(gcaps, caps)
    want_counts = np.bincount(outcome(ids, K3), minlength=2 * K3 + 2).astype(np.uint64)
    assert (want_counts[:K3 + 2] > 0).all() and want_counts[2 * K3 + 1] == 0    # three extractions, unmatched, exceptions of "ab"
    assert np.array_equal(gorp.count_outcomes(ids), want_counts)
    for m in range(1 << (2 * K3 + 1)):
        mask = np.array([(m >> b) & 1 for b in range(2 * K3 + 1)], np.uint8)
        check_selection(gorp, data, offsets, ids, mask, caps=caps)


# ---------------------------------------------------------------------------
# alignment: every source misalignment, every line length 0..80, destinations fenced by poison
# ---------------------------------------------------------------------------
def selection_patterns(n):
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
            "alternating": np.arange(n) % 2 == 0}
    for kept in range(1, 6):
        for dropped in range(1, 6):
            pats["%d kept / %d dropped" % (kept, dropped)] = np.arange(n) % (kept + dropped) < kept
    return pats


@pytest.mark.parametrize("mis", range(16))
def test_alignment_sweep_with_poisoned_destination(mis):
    import torch
    gorp = Gorp.construct(THREE)
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.permutation(81), rng.permutation(81)])          # every length 0..80, twice, in some order
    n = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(offsets[-1])
    payload = rng.integers(1, 255, total, dtype=np.uint8)
    d_off = torch.from_numpy(offsets.view(np.int32)).cuda()
    POISON, FENCE = 0xA5, 64
    want = np.array([1, 0, 0, 0, 0, 0, 0], np.uint8)                            # keep extraction 0, drop the unmatched
    src_buf = torch.empty(mis + total, dtype=torch.uint8, device="cuda")    # sized exactly: the batch ends where the tensor ends
    src_buf[mis:] = torch.from_numpy(payload).cuda()
    for dst_mis in (0, 3, 8, 13):
        for name, keep in selection_patterns(n).items():
            ids = np.where(keep, 0, -1).astype(np.int32)
            index, units, out_off, _ = restate(payload, offsets, ids, want, K3)
            d_ids = torch.from_numpy(ids).cuda()
            dst = torch.full((FENCE + dst_mis + len(units) + FENCE,), POISON, dtype=torch.uint8, device="cuda")
            d_index = torch.full((len(index) + 2,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
            d_ooff = torch.full((len(index) + 3,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
            got = gorp.select_lines_device(src_buf.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), None, want,
                                           out_index_ptr=d_index.data_ptr() + 4, out_data_ptr=dst.data_ptr() + FENCE + dst_mis,
                                           out_offsets_ptr=d_ooff.data_ptr() + 4, cap_lines=len(index), out_bytes_cap=len(units))
            where = (mis, dst_mis, name)
            assert got == (len(index), len(units)), where
            out = dst.cpu().numpy()
            assert (out[:FENCE + dst_mis] == POISON).all() and (out[FENCE + dst_mis + len(units):] == POISON).all(), where
            assert np.array_equal(out[FENCE + dst_mis:FENCE + dst_mis + len(units)], units), where
            oi, oo = d_index.cpu().numpy(), d_ooff.cpu().numpy()
            assert oi[0] == oi[-1] == 0x7FFFFFFF and np.array_equal(oi[1:-1].view(np.uint32), index), where
            assert oo[0] == oo[-1] == 0x7FFFFFFF and np.array_equal(oo[1:-1].view(np.uint32), out_off), where


# ---------------------------------------------------------------------------
# formats
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_id_formats_and_offset_widths(fmt, offsets_dtype):
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    lines = three_outcome_lines(3000, seed=23, max_len=250)                     # (u8 rows: offsets below 255)
    data, offsets = lines_to_csr(lines, offsets_dtype=offsets_dtype)
    ids, caps = orc.extract_batch(data, offsets)
    for want in ("unmatched", "exceptions", ["ab", "dee"], ["cee", "unmatched", "exceptions"]):
        mask = gorp.want_mask(want)
        if fmt == "int32":
            check_selection(gorp, data, offsets, ids, mask, caps=caps)
            check_selection(gorp, data, offsets, ids, mask)
        else:
            rows = pack_rows(ids, caps, np.uint16 if fmt == "u16" else np.uint8)
            got_rows, over = gorp.extract_batch(data, offsets, compact=1 if fmt == "u16" else 2)
            assert over == 0 and np.array_equal(got_rows, rows)
            check_selection(gorp, data, offsets, rows, mask)
            assert np.array_equal(gorp.count_outcomes(rows), restate(data, offsets, ids, mask, K3)[3])


def test_utf16_batch_with_units_above_0xff():
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
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
    gids, _ = gorp.extract_batch(data, offsets)
    assert np.array_equal(gids, ids)
    assert len(set(outcome(ids, K3).tolist())) >= 4
    for want in ("unmatched", "exceptions", "ab", ["cee", "dee", "unmatched"]):
        check_selection(gorp, data, offsets, ids, gorp.want_mask(want))


def test_lines_keep_their_terminators():
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    rng = random.Random(9)
    text = b"".join(ln.replace(b"\r", b"") + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in three_outcome_lines(1500, seed=4, max_len=120)) + b"a last line without one b"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    ref_off, ref_lines, _ = O.read_lines(text)
    assert np.array_equal(offsets, ref_off.astype(np.uint32))
    ids = np.array([orc.extract(ln)[0] for ln in ref_lines], np.int32)
    gids, _ = gorp.extract_batch(data, offsets, strip_eol=True)
    assert np.array_equal(gids, ids)
    for want in ("unmatched", ["ab", "cee"], ["ab", "cee", "dee", "unmatched", "exceptions"]):
        got = check_selection(gorp, data, offsets, ids, gorp.want_mask(want))
        assert got[1].tobytes() == b"".join(text[offsets[i]:offsets[i + 1]] for i in got[0])
    assert check_selection(gorp, data, offsets, ids, np.ones(7, np.uint8))[1].tobytes() == text


# ---------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK, 2 * SCAN_BLOCK + 1,
                               SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1])
def test_line_counts_around_tile_and_scan_boundaries(n):
    gorp = Gorp.construct(THREE)
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 40 if n < 100000 else 6, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = rng.integers(1, 255, int(offsets[-1]), dtype=np.uint8)
    ids = rng.choice(np.array([0, 1, 2, -1, -2, -3, -4], np.int32), n)
    for want in ("unmatched", [0, 2, "exceptions"]):
        check_selection(gorp, data, offsets, ids, gorp.want_mask(want))
    assert np.array_equal(gorp.count_outcomes(ids), np.bincount(outcome(ids, K3), minlength=8).astype(np.uint64))


def test_two_million_lines_on_the_device():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    K, n, L = 3, 2 * 1000 * 1000, 200
    data, offsets, cat = W.readme3_lines(n, seed=12, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)                              # (below 2^31: the same bits as uint32)
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    caps = torch.empty((n, 2 * gorp.max_groups), dtype=torch.int32, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
    assert torch.equal(ids, cat.to(torch.int32))
    oc = torch.where(ids >= 0, ids, torch.where(ids == -1, K, K + 1 + (-2 - ids))).long()
    counts = gorp.count_outcomes_device(ids.data_ptr(), n)
    assert np.array_equal(counts[:2 * K + 1], torch.bincount(oc, minlength=2 * K + 1).cpu().numpy().astype(np.uint64)) and counts[2 * K + 1] == 0
    for want in ("unmatched", "GetRequest", ["PutRequest", "GetRequest", "OtherRequest", "unmatched", "exceptions"]):
        mask = gorp.want_mask(want)
        keep = torch.from_numpy(mask.astype(bool)).cuda()[oc]
        index = keep.nonzero().flatten()
        k = int(index.numel())
        assert (k, k * L) == gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), None, mask)
        out = torch.empty(k * L, dtype=torch.uint8, device="cuda")
        o_index = torch.empty(k, dtype=torch.int32, device="cuda")
        o_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        o_ids = torch.empty(k, dtype=torch.int32, device="cuda")
        o_caps = torch.empty((k, caps.shape[1]), dtype=torch.int32, device="cuda")
        gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), mask, out_index_ptr=o_index.data_ptr(),
                                 out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(),
                                 out_caps_ptr=o_caps.data_ptr(), cap_lines=k, out_bytes_cap=k * L)
        assert torch.equal(o_index, index.to(torch.int32))
        assert torch.equal(out, data.view(n, L)[keep].reshape(-1))
        assert torch.equal(o_off, (torch.arange(k + 1, device="cuda") * L).to(torch.int32))
        assert torch.equal(o_ids, ids[keep]) and torch.equal(o_caps, caps[keep])


def test_syslog_200k_uneven_lines_64_rules():
    definition, meta = W.syslog_definition(64)
    gorp, orc = Gorp.construct(definition), oracle_for(definition)
    data, offsets, _ = W.syslog_lines(meta, 200000, seed=8, min_len=50, max_len=2000)
    ids, caps = orc.extract_batch(data, offsets, nthreads=16)
    K = 64
    assert np.array_equal(gorp.count_outcomes(ids), np.bincount(outcome(ids, K), minlength=2 * K + 2).astype(np.uint64))
    for want in ("unmatched", ["rule3", "rule40", 63], list(range(0, 64, 2)) + ["unmatched"]):
        check_selection(gorp, data, offsets, ids, gorp.want_mask(want), caps=caps)


# ---------------------------------------------------------------------------
# ids outside the range, capacity, stream order, round trip
# ---------------------------------------------------------------------------
def test_ids_outside_the_range_land_in_the_last_bin_and_are_never_selected():
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    lines = three_outcome_lines(4000, seed=31, max_len=200)
    data, offsets = lines_to_csr(lines)
    ids, caps = orc.extract_batch(data, offsets)
    rng = np.random.default_rng(2)
    for dtype, strays in ((np.uint16, [3, 77, 0x7FFF, -5, -100, -0x8000]), (np.uint8, [3, 77, 127, -5, -100, -128])):
        rows = pack_rows(ids, caps, dtype)
        hit = rng.random(len(ids)) < 0.05
        stray = rng.choice(np.array(strays, np.int64), len(ids))
        rows[hit, 0] = (stray[hit] & np.iinfo(dtype).max).astype(dtype)          # rows left unwritten hold whatever was there
        signed = rows[:, 0].astype(np.int16 if dtype == np.uint16 else np.int8).astype(np.int32)
        counts = gorp.count_outcomes(rows)
        assert counts[2 * K3 + 1] == hit.sum() > 0
        assert np.array_equal(counts, np.bincount(outcome(signed, K3), minlength=8).astype(np.uint64))
        got = check_selection(gorp, data, offsets, rows, np.ones(2 * K3 + 1, np.uint8))
        assert len(got[0]) == len(ids) - hit.sum() and not hit[got[0]].any()
    wide = ids.copy()
    wide[hit] = rng.choice(np.array([3, 12345, -5, -2 ** 31, 2 ** 31 - 1], np.int64), int(hit.sum())).astype(np.int32)
    assert gorp.count_outcomes(wide)[2 * K3 + 1] == hit.sum()
    got = check_selection(gorp, data, offsets, wide, np.ones(2 * K3 + 1, np.uint8))
    assert not hit[got[0]].any()


def test_capacity_too_small_writes_nothing_and_size_query_equals_run():
    import torch
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    lines = three_outcome_lines(3000, seed=41, max_len=300)
    data, offsets = lines_to_csr(lines)
    ids, caps = orc.extract_batch(data, offsets)
    mask = gorp.want_mask(["unmatched", "exceptions"])
    index, units, out_off, _ = restate(data, offsets, ids, mask, K3)
    k, nbytes = len(index), len(units)
    d = {name: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in
         (("data", data.copy()), ("off", offsets), ("ids", ids), ("caps", caps))}
    inputs = (d["data"].data_ptr(), d["off"].data_ptr(), len(ids), d["ids"].data_ptr(), d["caps"].data_ptr(), mask)
    assert gorp.select_lines_device(*inputs) == (k, nbytes)                      # the size query
    POISON = 0x5A
    outs = {"out_index_ptr": torch.full((k,), POISON, dtype=torch.uint8, device="cuda").repeat(4), "out_data_ptr": torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda"),
            "out_offsets_ptr": torch.full((4 * (k + 1),), POISON, dtype=torch.uint8, device="cuda"), "out_ids_ptr": torch.full((4 * k,), POISON, dtype=torch.uint8, device="cuda"),
            "out_caps_ptr": torch.full((4 * k * caps.shape[1],), POISON, dtype=torch.uint8, device="cuda")}
    ptrs = {name: t.data_ptr() for name, t in outs.items()}
    L = N.lib()
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    for cap_lines, cap_bytes in ((k - 1, nbytes), (k, nbytes - 1), (0, 0)):
        sizes = (C.c_uint64(0), C.c_uint64(0))
        rc = L.gx_select_lines(gorp._h.ptr, *inputs[:5], mask.ctypes.data, ptrs["out_index_ptr"], ptrs["out_data_ptr"], ptrs["out_offsets_ptr"],
                               ptrs["out_ids_ptr"], ptrs["out_caps_ptr"], cap_lines, cap_bytes, C.byref(sizes[0]), C.byref(sizes[1]), C.byref(o))
        assert rc == N.GX_E_LIMIT and "smaller than" in N.last_error()
        assert (sizes[0].value, sizes[1].value) == (k, nbytes)
        for t in outs.values():
            assert bool((t == POISON).all())
    with pytest.raises(GorpError) as ei:
        gorp.select_lines_device(*inputs, cap_lines=k - 1, out_bytes_cap=nbytes, **ptrs)
    assert ei.value.code == N.GX_E_LIMIT
    assert gorp.select_lines_device(*inputs, cap_lines=k, out_bytes_cap=nbytes, **ptrs) == (k, nbytes)
    assert np.array_equal(outs["out_data_ptr"].cpu().numpy(), units)
    assert np.array_equal(outs["out_index_ptr"].cpu().numpy().view(np.uint32), index)
    assert np.array_equal(outs["out_offsets_ptr"].cpu().numpy().view(np.uint32), out_off)
    assert np.array_equal(outs["out_ids_ptr"].cpu().numpy().view(np.int32), ids[index])
    assert np.array_equal(outs["out_caps_ptr"].cpu().numpy().view(np.int32).reshape(k, -1), caps[index])


def test_selection_follows_a_no_sync_batch_on_its_stream():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L, K = 300000, 200, 3
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.full((n, width), 0x55, dtype=torch.uint8, device="cuda")       # ids nobody wrote: outcome 2K + 1
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    mask = gorp.want_mask("unmatched")
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True,
                                  compact=2, line_bytes_hint=L)
        k, nbytes = gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, mask, compact=2, stream=stream.cuda_stream)
        counts = gorp.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=stream.cuda_stream)
        index = torch.empty(k, dtype=torch.int32, device="cuda")
        gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, mask, out_index_ptr=index.data_ptr(), cap_lines=k,
                                 compact=2, stream=stream.cuda_stream, no_sync=True)
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, mask, out_data_ptr=out.data_ptr(), out_bytes_cap=nbytes,
                                 compact=2, stream=stream.cuda_stream, no_sync=True)
    # the copy pass of that last call may still be reading the handle's workspace: calls on ANOTHER stream wait for it before they
    # lay out their own, and neither result suffers
    other = torch.cuda.Stream()
    gets = gorp.want_mask("GetRequest")
    with torch.cuda.stream(other):
        counts2 = gorp.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=other.cuda_stream)
        k2, _ = gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, gets, compact=2, stream=other.cuda_stream)
        index2 = torch.empty(k2, dtype=torch.int32, device="cuda")
        gorp.select_lines_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, gets, out_index_ptr=index2.data_ptr(), cap_lines=k2,
                                 compact=2, stream=other.cuda_stream)
    stream.synchronize()
    want_index = (cat == -1).nonzero().flatten()
    assert k == want_index.numel() > 0 and nbytes == k * L and counts[2 * K + 1] == 0 and counts[K] == k
    assert torch.equal(index, want_index.to(torch.int32))
    assert torch.equal(out, data.view(n, L)[cat == -1].reshape(-1))
    assert np.array_equal(counts2, counts) and torch.equal(index2, (cat == 1).nonzero().flatten().to(torch.int32))


def test_selected_batch_extracts_to_the_selected_rows():
    gorp, orc = Gorp.construct(THREE), oracle_for(THREE)
    lines = three_outcome_lines(4000, seed=51)
    data, offsets = lines_to_csr(lines)
    ids, caps = orc.extract_batch(data, offsets)
    for want in (["ab", "dee"], ["cee", "exceptions"], "unmatched"):
        index, sdata, soff, sids, scaps = check_selection(gorp, data, offsets, ids, gorp.want_mask(want), caps=caps)
        again_ids, again_caps = gorp.extract_batch(sdata, soff)
        assert np.array_equal(again_ids, sids) and np.array_equal(again_caps, scaps)
        text = gorp.results_to_jsonl(sdata, soff, sids, scaps, id_as="id")
        assert text == gorp.results_to_jsonl(data, offsets, np.where(np.isin(np.arange(len(ids)), index), ids, -1).astype(np.int32), caps, id_as="id")


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------
def test_text_select_is_what_text_to_jsonl_drops():
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    orc = oracle_for(W.readme3_definition())
    K = 3
    data, offsets, cat = W.readme3_lines(20000, seed=61)
    d, o = data.numpy(), offsets.numpy().astype(np.int64)
    rng = random.Random(6)
    text = b"".join(bytes(d[o[i]:o[i + 1]]) + rng.choice([b"\n", b"\n", b"\r\n"]) for i in range(len(o) - 1)) + b"[123456789]: GET 5ms /tail"
    ref_off, ref_lines, _ = O.read_lines(text)
    ids = np.array([orc.extract(ln)[0] for ln in ref_lines], np.int32)
    jsonl, n_lines, n_matched, n_exceptions = gorp.text_to_jsonl(text, id_as="rule")
    dropped, counts, n_lines2 = gorp.text_select(text, ("unmatched", "exceptions"))
    assert n_lines == n_lines2 == len(ref_lines)
    assert jsonl.count(b"\n") + len(dropped.splitlines()) == n_lines
    index, units, _, want_counts = restate(np.frombuffer(text, dtype=np.uint8), ref_off, ids, gorp.want_mask(("unmatched", "exceptions")), K)
    assert 0 < len(index) < n_lines and dropped == units.tobytes()
    assert np.array_equal(counts, want_counts) and counts[:K].sum() == n_matched and counts[K + 1:2 * K + 1].sum() == n_exceptions
    gets, _, _ = gorp.text_select(text, "GetRequest")
    assert gets == restate(np.frombuffer(text, dtype=np.uint8), ref_off, ids, gorp.want_mask("GetRequest"), K)[1].tobytes()
    assert gorp.text_select(b"", "unmatched")[0] == b""
