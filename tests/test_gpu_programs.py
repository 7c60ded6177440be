"""GPU tests of extractions RUN as programs (gx_kernels.hip: pike_capture, the Pike VM of the per-line kernel).

GX_CREATE_PROGRAMS makes every extraction of a definition keep its program, so the VM, its thread lists in device memory, the
lane slots and every API path around them are driven by the definitions and generators the rest of the suite uses, not by the one
family (blank-separated \\S* fields) that is too ambiguous for an automaton.  Everything is compared exactly: with the CPU oracle
(backtracking, java.util.regex restated) and, where the same definition has a handle without the flag, with that handle too."""
import random

import numpy as np
import pytest

import test_compiler_vs_oracle as TC
import test_gpu_select as TS
import test_gpu_utf8 as TU
from blob_interp import Blob
from gorp_amd import _native as N
from gorp_amd import gorp as G
from gorp_amd import workloads as W
from gorp_amd.gorp import CookedExtraction, ExtractionException, Gorp, lines_to_csr
from oracle import oracle as O
from test_gpu_parity import check_batch, check_cooked_match, fl, oracle_for
from test_gpu_utf8 import byte_map  # noqa: F401  (the fixture: unit -> byte map of gx_utf8.hpp, from the CPU)

pytestmark = pytest.mark.gpu

PROGRAMS = N.GX_CREATE_PROGRAMS
BLOCKS = 35    # gx_stat: workgroups a per-line launch of the handle is kept within


def as_programs(definition):
    gorp = Gorp.construct(definition, flags=PROGRAMS)
    assert gorp.stat(27) == len(definition) and gorp.stat(7) == 0 and 1 <= gorp.stat(BLOCKS) <= 64
    return gorp


def same_as_plain(flagged, plain, lines):
    """Dense rows of both handles on one batch: equal."""
    assert plain.stat(27) == 0 and plain.stat(BLOCKS) == -1
    data, offsets = lines_to_csr(lines)
    fm, fc = flagged.extract_batch(data, offsets)
    pm, pc = plain.extract_batch(data, offsets)
    assert np.array_equal(fm, pm) and np.array_equal(fc, pc)


# ---------------------------------------------------------------------------
# the generators of the CPU differential tests, through the device's VM
# ---------------------------------------------------------------------------
def test_random_definitions_as_programs():
    """test_random_definitions_through_kernels with the flag: 60 definitions (1-4 extractions each), 20 random lines and 44 sampled
    from the match automaton per definition, every result format.  Seed 4321 gives 1 721 matched lines and 243 exceptions (counted with the oracle alone, on the CPU)."""
    rng = random.Random(4321)
    n_defs = n_hits = n_exc = 0
    tally = {}
    while n_defs < 60:
        exts = [{"name": "e%d" % i, "pieces": TC.gen_pieces(rng)} for i in range(rng.randint(1, 4))]
        pair = TC.construct_both(lambda: as_programs(fl(exts)), lambda: oracle_for(fl(exts)), tally)
        if pair is None:
            continue
        gorp, orc = pair
        n_defs += 1
        b = Blob(gorp.blob())
        assert all(b.is_pike(k) for k in range(len(exts))) and not b.union_ok
        lines = [TC.gen_line(rng) for _ in range(20)] + [TC.sample_from_match_automaton(b, rng) for _ in range(44)]
        mid, _ = check_batch(gorp, orc, lines)
        same_as_plain(gorp, Gorp.construct(fl(exts)), lines)
        n_hits += int((mid >= 0).sum())
        n_exc += int((mid <= -2).sum())
    print("random definitions as programs: matched %d, exceptions %d" % (n_hits, n_exc))
    assert n_hits >= 600
    assert tally.get("product_only", 0) == 0 and tally.get("oracle_only", 0) == 0, tally


def raw_gorp(pattern, flags):
    """One extraction from a raw regexp pair: '.*' lets every line through the matcher, the capture regexp decides."""
    h = G._create([".*"], [pattern], flags)
    groups = N.lib().gx_num_groups(h.ptr, 0)
    return Gorp(h, [CookedExtraction(0, "raw", pattern, ["g%d" % g for g in range(groups)])])


def test_random_raw_patterns_as_programs():
    """test_random_raw_regex_pairs_capture_parity's patterns on the device: lazy against greedy quantifiers (SPLIT with the branches
    swapped), alternation order, counted repetitions, groups under quantifiers and alternations, groups that stay unset (the
    `pb < 0 || pe < 0` branch), and -- the matcher being '.*' -- the program refusing a line the automaton let through: id -2.
    Seed 99, 150 patterns: 750 matched lines, 102 of them with an unset group, 2 093 refused (counted with the oracle alone, on the CPU)."""
    rng = random.Random(99)
    n = matched = unset = refused = 0
    while n < 150:
        pat = TC.gen_pattern(rng, lazy=True)
        try:
            gorp = raw_gorp(pat, PROGRAMS)
            orc = O.OracleGorp([".*"], [pat])
        except (O.OracleError, G.DefinitionParseException):
            continue
        n += 1
        assert gorp.stat(27) == 1
        lines = [TC.gen_line(rng) for _ in range(15)] + TC._sample_accepted(rng, pat)
        mid, caps = check_batch(gorp, orc, lines)
        same_as_plain(gorp, raw_gorp(pat, 0), lines)
        hit = mid >= 0
        matched += int(hit.sum())
        refused += int((mid == -2).sum())
        unset += int((hit & (caps[:, :2 * gorp.num_groups(0)] < 0).any(axis=1)).sum())
    print("raw patterns as programs: matched %d, with an unset group %d, refused %d" % (matched, unset, refused))
    assert matched >= 200
    assert unset >= 20
    assert refused >= 200     # (a tenth of the oracle's count)


# ---------------------------------------------------------------------------
# outcomes
# ---------------------------------------------------------------------------
def test_all_three_outcomes_from_programs():
    """Matched, unmatched and ExtractionException (-2 - k: the program says no where the match automaton said yes) from programs,
    counted on the device, and the one-line calls' exception text."""
    gorp, plain, orc = as_programs(TS.THREE), Gorp.construct(TS.THREE), oracle_for(TS.THREE)
    lines = TS.three_outcome_lines(2000, seed=11, max_len=300) + [b"a\rb", b"a\r\rb", b"a" + b"x" * 40 + b"\rb", b"ab", b"a\r", b"", b"c\r"]
    lines = [ln.decode("latin-1") for ln in lines]
    mid, caps = check_batch(gorp, orc, lines)
    same_as_plain(gorp, plain, lines)
    want = np.bincount(TS.outcome(mid, TS.K3), minlength=2 * TS.K3 + 2).astype(np.uint64)
    print("three outcomes from programs: counts per outcome index %s" % want.tolist())
    assert (want[:TS.K3 + 2] > 0).all() and want[TS.K3 + 1] >= 100     # every extraction, unmatched, exceptions of "ab"
    data, offsets = lines_to_csr(lines)
    rows, _ = gorp.extract_batch(data, offsets, compact=True)
    for ids in (mid, rows):
        assert np.array_equal(gorp.count_outcomes(ids), want) and np.array_equal(plain.count_outcomes(ids), want)
    # the one-line calls (tests/test_gpu_parity.py: test_exception_null_and_safe)
    assert gorp.extract("a--b").asMap() == {"x": "--"}
    assert gorp.extract("zzz") is None
    with pytest.raises(ExtractionException, match=r"Internal error: high-level match for extraction #0 \(ab\) failed"):
        gorp.extract("a\rb")
    assert gorp.extractSafe("a\rb") is None
    assert gorp.extractSafe("a--b").asMap() == {"x": "--"}


# ---------------------------------------------------------------------------
# the one-line calls (k_extract_one: the lane slot behind the batch kernels' 256 * blocks)
# ---------------------------------------------------------------------------
def test_golden_vectors_through_the_one_line_calls(golden):
    hit = miss = 0
    for t in golden("full_extraction")["tests"]:
        gorp = as_programs(fl(t["extractions"]))
        for c in t["cases"]:
            result = gorp.extract(c["input"])
            assert result is not None
            if c.get("not_null"):
                continue
            assert result.getId() == c["id"]
            stuff = result.asMap(c.get("id_as"))
            for k, v in c["map"].items():
                assert stuff[k] == v
            if "map_size" in c:
                assert len(stuff) == c["map_size"]
        h, m = check_cooked_match(gorp, [c["input"] for c in t["cases"]])
        hit, miss = hit + h, miss + m
    g = golden("configs")
    for key in ("simple_grp", "readme_3"):
        gorp = as_programs(fl(g[key]["extractions"]))
        for c in g[key]["cases"]:
            assert gorp.getMatcher().match(c["input"]) == c["match"]
            r = gorp.extract(c["input"])
            if not c["match"]:
                assert r is None
            else:
                assert r.getId() == c["id"]
                for k, v in c.get("map", {}).items():
                    assert r.asMap()[k] == v
        h, m = check_cooked_match(gorp, [c["input"] for c in g[key]["cases"]])
        hit, miss = hit + h, miss + m
    print("golden vectors: CookedExtraction.match matched %d times, null %d times" % (hit, miss))
    assert (hit, miss) == (15, 18)     # (what the oracle alone gives for these vectors)


# ---------------------------------------------------------------------------
# 16-bit code units and UTF-8
# ---------------------------------------------------------------------------
def test_utf16_units_and_utf8_lines_as_programs(byte_map):  # noqa: F811
    """CH = uint16_t in pike_capture and class_of's search for units above 0xFF; the UTF-8 modes walk the flagged lines as Strings and
    map the program's offsets back to bytes.  The "ab" extraction refuses a line with U+2028 inside: -2 - 3."""
    gorp, plain, orc = as_programs(TU.UNI), Gorp.construct(TU.UNI), oracle_for(TU.UNI)
    lines = TU.uni_lines(1500, seed=7) + [b"", TU.ZHONG, b"a" + "\u2028".encode() + b"b", "k=é中x 中".encode()]
    ids, caps_units = TU.oracle_rows(orc, lines, 2 * gorp.max_groups)
    caps_bytes = TU.to_byte_offsets(caps_units, lines, byte_map(lines))
    wide = sum(1 for ln in lines if any(u > 0xFF for u in TU.units_of(ln)))
    print("utf: %d lines, %d with a unit above 0xFF, ids %s" % (len(lines), wide, np.unique(ids, return_counts=True)))
    assert (ids == -5).sum() >= 10 and wide >= 100 and all((ids == k).sum() >= 10 for k in range(4))
    # a UTF-16 batch: the Strings' code units
    units = [TU.units_of(ln) for ln in lines]
    u_off = np.zeros(len(lines) + 1, np.uint32)
    u_off[1:] = np.cumsum([len(u) for u in units])
    u_data = np.concatenate(units)
    for handle in (gorp, plain):
        m, c = handle.extract_batch(u_data, u_off)
        assert np.array_equal(m, ids) and np.array_equal(c, caps_units)
    rows, over = gorp.extract_batch(u_data, u_off, compact=1)
    m, c = G.unpack_rows(rows)
    assert over == 0 and np.array_equal(m, ids) and np.array_equal(c, caps_units)
    # UTF-8 bytes, offsets in bytes and in units, dense and u16 rows
    data, offsets = lines_to_csr(lines)
    for mode, want in (("bytes", caps_bytes), ("units", caps_units)):
        for handle in (gorp, plain):
            m, c = handle.extract_batch(data, offsets, utf8=mode)
            assert handle.stat(33) == TU.n_flagged(lines)
            assert np.array_equal(m, ids) and np.array_equal(c, want)
        rows, over = gorp.extract_batch(data, offsets, utf8=mode, compact=1)
        m, c = G.unpack_rows(rows)
        assert over == 0 and np.array_equal(m, ids) and np.array_equal(c, want)


# ---------------------------------------------------------------------------
# a lane's thread lists, reused for the lines of its stride
# ---------------------------------------------------------------------------
def test_thread_lists_reused_across_a_lanes_lines():
    """Device pointers and more lines than lanes: lane q takes lines q, q + 256 blocks, q + 512 blocks, ... with ONE set of thread
    lists.  Its lines differ in length and outcome (a 180-byte match, a 12-byte match, no match, empty -- in that order, started at a
    seeded place of the cycle), so marks, generation counters or boundaries left by a longer line would show in the next."""
    import torch
    gorp, orc = as_programs(W.readme3_definition()), oracle_for(W.readme3_definition())
    blocks = gorp.stat(BLOCKS)
    stride = 256 * blocks
    n = 3 * stride + 77
    rng = random.Random(5)
    start = [rng.randrange(4) for _ in range(stride)]
    verbs = ["GET", "PUT", "POST"]
    lines = []
    for i in range(n):
        kind = (start[i % stride] + i // stride) % 4
        if kind == 0:
            head = "[%d]: %s %dms /" % (100000000 + i, verbs[i % 3], i % 5000)
            lines.append(head + "p" * (180 - len(head)))
        elif kind == 1:
            lines.append("[%d]: %s %dms /" % (i % 10, "XGP"[i % 3], i % 10))
        elif kind == 2:
            lines.append(["[%d]: GET %dms" % (i, i % 100), "nope %d" % i, "[12]: GET 5ms /x y" + "z" * (i % 50)][i % 3])
        else:
            lines.append("")
    assert len(lines[start.index(0)]) == 180 and 12 in {len(ln) for ln in lines}
    data, offsets = lines_to_csr(lines)
    omid, ocaps = orc.extract_batch(data, offsets, nthreads=8)
    print("lane reuse: blocks %d, %d lines, matched %d" % (blocks, n, int((omid >= 0).sum())))
    assert all((omid == k).sum() > 4000 for k in (-1, 0, 1, 2))
    d, o = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    second = torch.cuda.Stream()
    outs = [(torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, 2 * gorp.max_groups), -7, dtype=torch.int32, device="cuda"))
            for _ in range(2)]
    torch.cuda.synchronize()
    gorp.extract_batch_device(d.data_ptr(), o.data_ptr(), n, outs[0][0].data_ptr(), outs[0][1].data_ptr())
    gorp.extract_batch_device(d.data_ptr(), o.data_ptr(), n, outs[1][0].data_ptr(), outs[1][1].data_ptr(), stream=second.cuda_stream, no_sync=True)
    second.synchronize()
    torch.cuda.synchronize()
    for mid, caps in outs:
        assert np.array_equal(mid.cpu().numpy(), omid) and np.array_equal(caps.cpu().numpy(), ocaps)


def test_fewer_workgroups_than_64():
    """64 extractions of up to 154 instructions and 10 groups: the thread lists of 64 workgroups would pass the scratch budget, so the
    per-line launches are kept within fewer (gx_stat 35) and every lane takes several lines."""
    rules, meta = W.syslog_definition(64, seed=3)
    gorp, plain, orc = as_programs(rules), Gorp.construct(rules), oracle_for(rules)
    blocks = gorp.stat(BLOCKS)
    print("64 extractions as programs: blocks %d" % blocks)
    assert 1 <= blocks < 64
    data, offsets, _ = W.syslog_lines(meta, 20000, seed=41, corrupt_frac=0.1)
    assert len(offsets) - 1 > 2 * 256 * blocks
    omid, ocaps = orc.extract_batch(data, offsets, nthreads=16)
    assert (omid >= 0).sum() > 15000 and (omid == -1).sum() > 500 and len(np.unique(omid[omid >= 0])) == 64
    mid, caps = gorp.extract_batch(data, offsets)
    assert np.array_equal(mid, omid) and np.array_equal(caps, ocaps)
    rows, over = gorp.extract_batch(data, offsets, compact=True)
    cm, cc = G.unpack_rows(rows)
    assert over == 0 and np.array_equal(cm, omid) and np.array_equal(cc, ocaps)
    pm, pc = plain.extract_batch(data, offsets)
    assert np.array_equal(pm, omid) and np.array_equal(pc, ocaps)
    m2, _ = gorp.extract_batch(data, offsets, match_only=True)
    assert np.array_equal(m2, orc.extract_batch(data, offsets, nthreads=16, match_only=True)[0])


# ---------------------------------------------------------------------------
# long lines
# ---------------------------------------------------------------------------
def test_long_lines_as_programs():
    """Lines at the edge of the one-line kernel's 16 384 units and beyond it (the batch path on a device copy), offsets above 65 534
    and 254 in the compact rows, and -- through CookedExtraction.match, which runs a program without the matcher in front of it --
    long lines on which every thread dies in the first bytes or at the very last one."""
    gorp, orc = as_programs(W.readme3_definition()), oracle_for(W.readme3_definition())
    head = "[123456789]: GET 12ms /"

    def of_length(units):
        return head + "p" * (units - len(head)) if units >= len(head) + 1 else "x" * units
    lines = [of_length(u) for u in (0, 1, 16384, 16385, 70000)]
    assert [len(ln) for ln in lines] == [0, 1, 16384, 16385, 70000]
    dies_first = "#" + of_length(20000)                    # no thread survives the first unit
    dies_last = of_length(20000) + " "                     # \S+ was the last piece: the blank ends every thread
    put_70000 = "[1]: PUT 7ms /" + "q" * (70000 - 14)
    lines += [dies_first, dies_last, put_70000, "[1]: X 1ms /"]
    for ln in lines:
        want = orc.extract(ln)
        r = gorp.extract(ln)
        assert (r is None) == (want[0] < 0), len(ln)
        if r is not None:
            assert r.getId() == gorp.getExtractions()[want[0]].getName()
            assert [r.asMap()[name] for name in ("timestamp", "verb", "timeTakenInMsec", "path")] == [ln[b:e] for b, e in want[1]]
    mid, caps = check_batch(gorp, orc, lines)
    assert mid.tolist() == [-1, -1, 1, 1, 1, -1, -1, 0, 2]
    assert caps[4].tolist()[-1] == 70000 and caps[7].tolist()[-1] == 70000     # (one offset each beyond the u16 rows, more beyond the u8 rows)
    hit, miss = check_cooked_match(gorp, [dies_first, dies_last, lines[2], lines[3], "[1]: X 1ms /", ""])
    assert hit == 2 + 2 + 1 and miss == 18 - hit    # the two GET lines: GetRequest and OtherRequest; "X": OtherRequest alone


# ---------------------------------------------------------------------------
# the whole-file calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("utf8", [False, True])
def test_whole_file_calls_as_programs(utf8):
    """Raw text -> split pass, strip_eol, extraction, JSON Lines / selection / partition, on a handle whose extractions are programs:
    byte for byte what the handle without the flag gives, counts included, and the counts the oracle gives for the lines."""
    gorp, plain, orc = as_programs(TS.THREE), Gorp.construct(TS.THREE), oracle_for(TS.THREE)
    # inside a line, what '.' refuses and the automaton dialect's '.' takes: NEL as a Latin-1 unit, U+2028 in UTF-8 (a '\r' would end the line)
    inner = "\u2028".encode() if utf8 else b"\x85"
    lines = [ln.replace(b"\r", inner) for ln in TS.three_outcome_lines(5000, seed=17, max_len=300)]
    rng = random.Random(18)
    lines[-1] += b"tail"                                  # (the last line: no terminator)
    # (a lone '\r' in front of an empty line's '\n' would be one terminator, and one line fewer)
    text = b"".join(ln + rng.choice([b"\n", b"\r\n", b"\r"] if nxt else [b"\n", b"\r\n"]) for ln, nxt in zip(lines[:-1], lines[1:])) + lines[-1]
    _, kept, _ = O.read_lines(text)
    assert kept == lines
    ids = np.array([orc.extract(ln.decode("utf-8" if utf8 else "latin-1"))[0] for ln in kept], np.int32)
    want = np.bincount(TS.outcome(ids, TS.K3), minlength=2 * TS.K3 + 2).astype(np.uint64)
    print("whole-file calls (utf8=%s): %d lines, counts per outcome index %s" % (utf8, len(kept), want.tolist()))
    assert (want[:TS.K3 + 2] > 0).all() and want[TS.K3 + 1] >= 200
    got = [h.text_to_jsonl(text, id_as="rule", utf8=utf8) for h in (gorp, plain)]
    assert got[0] == got[1]
    assert got[0][1:] == (len(kept), int((ids >= 0).sum()), int((ids <= -2).sum()))
    got = [h.text_select(text, ("unmatched", "exceptions"), utf8=utf8) for h in (gorp, plain)]
    assert got[0][0] == got[1][0] and got[0][2] == got[1][2] == len(kept)
    assert np.array_equal(got[0][1], want) and np.array_equal(got[1][1], want)
    got = [h.text_to_jsonl_by_extraction(text, id_as="rule", utf8=utf8) for h in (gorp, plain)]
    assert got[0][0] == got[1][0] and got[0][3] == got[1][3] == len(kept)
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], want) and np.array_equal(got[1][2], want)
