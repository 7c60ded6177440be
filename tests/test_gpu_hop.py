"""The hop tier's kernels (gx_hop_dev.hpp's walk in the tile kernel, gx_tile_hop*.hip, and in the hop slice kernel, gx_kernels.hip)
where the suite had not looked: definitions other than the syslog family, records out of LDS on such definitions, cut lines lying
next to the bytes they were cut from, runs of every length at every window offset, and the tile kernel's walk WITH second chances,
which a wave only takes for the tile after one that wanted them.  Every comparison is bit-exact against the oracle; every test that
means a hop kernel asserts that the launch took one (gx_stat 25).  tests/test_hop_host.py pins the preconditions on the CPU."""
import random

import numpy as np
import pytest

import hop_cases as HC
from gorp_amd import _native as N
from gorp_amd import gorp as G
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, lines_to_csr
from oracle import oracle as O
from test_gpu_parity import _tiled_on_device, check_batch, fl, oracle_for

pytestmark = pytest.mark.gpu

AUTO, HOPS, HOP_SLICES = N.GX_KERNEL_AUTO, N.GX_KERNEL_HOPS, N.GX_KERNEL_HOP_SLICES
TOOK = {AUTO: (HOPS, HOP_SLICES), HOPS: (HOPS,), HOP_SLICES: (HOP_SLICES,)}   # gx_stat(h, 25) after a launch that asked for the key


def match_only_ids(omid):
    """What a match-only batch reports: the first accepting extraction (an ExtractionException's -2-k is extraction k there)."""
    return np.where(omid <= -2, -2 - omid, omid)


def assert_rows(what, lines, mid, caps, omid, ocaps):
    """Bit-exact, and the first line that differs in the message."""
    bad = mid != omid
    if caps is not None:
        bad = bad | (caps != ocaps).any(axis=1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d lines differ; first: line %d %r: id %d, want %d; offsets %s, want %s" % (
            what, int(bad.sum()), len(bad), i, lines[i] if lines is not None else None, mid[i], omid[i],
            None if caps is None else caps[i].tolist(), None if caps is None else ocaps[i].tolist()))


def check_hop_kernels(gorp, lines, data, offsets, omid, ocaps, kernels=(HOPS, HOP_SLICES), compact=False, **kw):
    """A batch through the named hop kernels: captures (where the fused automaton has hop tables) as dense rows -- and as u16 and u8 rows
    with compact=True -- and match only (the match automaton's tables).  Each launch must have taken the kernel."""
    assert gorp.stat(22) > 0
    for kernel in kernels:
        if gorp.stat(14) > 0:
            mid, caps = gorp.extract_batch(data, offsets, kernel=kernel, **kw)
            assert gorp.stat(25) in TOOK[kernel], (kernel, gorp.stat(25))
            assert_rows("kernel %d" % kernel, lines, mid, caps, omid, ocaps)
            for form, limit in ((1, 65534), (2, 254)) if compact else ():
                if form == 2 and len(gorp.getExtractions()) > 126:
                    continue
                rows, over = gorp.extract_batch(data, offsets, kernel=kernel, compact=form, **kw)
                assert gorp.stat(25) in TOOK[kernel], (kernel, gorp.stat(25))
                cm, cc = G.unpack_rows(rows)
                big = ocaps > limit
                assert over == int(big.sum()), (kernel, form)
                assert_rows("kernel %d, rows %d" % (kernel, form), lines, cm, cc, omid, np.where(big, limit, ocaps))
        mo, _ = gorp.extract_batch(data, offsets, kernel=kernel, match_only=True, **kw)
        assert gorp.stat(25) in TOOK[kernel], (kernel, gorp.stat(25))
        assert_rows("kernel %d, match only" % kernel, lines, mo, None, match_only_ids(omid), None)


def answers(orc, lines):
    data, offsets = lines_to_csr(lines)
    omid, ocaps = orc.extract_batch(data, offsets, nthreads=8)
    return data, offsets, omid, ocaps


def test_random_definitions_through_the_hop_kernels():
    """test_random_definitions_through_kernels' definitions again, with GX_CREATE_TIER_HOP: their dense rows fit LDS, so without the flag
    no hop kernel ever saw them.  About 200 lines each (more than three tiles: the lanes of a wave sit in unlike states): random
    text, walks of the match automaton, and both damaged; through check_batch, and as dense, u16 and u8 rows and match only through
    the default choice, the tile kernel and the hop slice kernel, each launch shown to have taken a hop kernel.  Match-only always runs a hop kernel (the match automaton always has its image); captures
    do for the definitions whose capture programs the tier takes -- more than half, or this test would be testing other kernels."""
    import test_compiler_vs_oracle as TC
    from blob_interp import Blob
    rng = random.Random(4321)
    n_defs = n_hop = n_hits = n_lines = 0
    tally = {}
    while n_defs < 150:
        exts = [{"name": "e%d" % i, "pieces": TC.gen_pieces(rng)} for i in range(rng.randint(1, 4))]
        pair = TC.construct_both(lambda: Gorp.construct(fl(exts), flags=N.GX_CREATE_TIER_HOP), lambda: oracle_for(fl(exts)), tally)
        if pair is None:
            continue
        gorp, orc = pair
        n_defs += 1
        assert gorp.stat(26) in (0, 2) and gorp.stat(22) > 0, (exts, gorp.stat(26))
        b = Blob(gorp.blob())
        lines = [TC.gen_line(rng) for _ in range(60)] + [TC.sample_from_match_automaton(b, rng) for _ in range(100)]
        lines += [HC.damage(rng, rng.choice(lines)) for _ in range(40)]
        check_batch(gorp, orc, lines)
        assert gorp.stat(25) in TOOK[AUTO], (exts, gorp.stat(25))     # (check_batch ends on a match-only batch)
        data, offsets, omid, ocaps = answers(orc, lines)
        n_hop += gorp.stat(14) > 0
        try:      # (every row form again through each choice of kernel, the launch's kernel asserted after each)
            check_hop_kernels(gorp, lines, data, offsets, omid, ocaps, kernels=(AUTO, HOPS, HOP_SLICES), compact=True)
        except AssertionError as e:
            raise AssertionError("%s\ndefinition: %r" % (e, exts))
        n_lines += len(lines)
        n_hits += int((omid >= 0).sum())
    print("definitions with hop tables for captures: %d of %d; lines matched: %d of %d" % (n_hop, n_defs, n_hits, n_lines))
    assert 2 * n_hop > n_defs, (n_hop, n_defs)
    assert 10 * n_hits > n_lines, (n_hits, n_lines)      # (a tenth; test_random_definitions_through_kernels asks 1 500 of 9 600)
    assert tally.get("product_only", 0) == 0 and tally.get("oracle_only", 0) == 0, tally


def _terminated(rng, lines):
    """(raw text, line offsets, the lines a reader sees) of the lines that hold no terminator themselves."""
    raw = b"".join(ln.encode("latin-1") + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in lines if "\r" not in ln and "\n" not in ln)
    off, _ = G.split_lines(raw)
    _, want_lines, _ = O.read_lines(raw)
    return raw, off, want_lines


@pytest.mark.parametrize("n_ext", [8, 48, 400])
def test_fielded_definitions_on_both_hop_kernels(n_ext):
    """Fielded definitions (tests/hop_cases.py) of 8, 48 and 400 extractions: fields, separators, loop sets and tail sets no syslog
    definition has.  At 400 neither kernel has every reachable state's record in LDS: the walk that keeps a record while its lane stays
    in the state and fetches the others from global memory, on text other than syslog.  Lines in the heaviest interval, over all
    intervals, with bytes above 0x7F, and a quarter damaged; dense / u16 / u8 rows, match only, terminated text; lines of 50-2000
    bytes announced as uneven through the hop slice kernel; one UTF-16 batch through the tile kernel's UTF-16 build with a unit
    above 0xFF inside a value."""
    rules, makers, rng = HC.fielded(n_ext, 1)
    gorp, orc = Gorp.construct(rules, flags=N.GX_CREATE_TIER_HOP), oracle_for(rules)
    assert gorp.stat(26) == 0 and gorp.stat(14) > 0
    if n_ext == 400:
        assert gorp.stat(16) > gorp.stat(15) and gorp.stat(21) < gorp.stat(15)     # records out of LDS in both kernels
    else:
        assert gorp.stat(16) == gorp.stat(15) and gorp.stat(17) > 0
    lines = []
    for i in range(3000):
        ln = makers[rng.randrange(n_ext)](rng, style=("lower", "mixed", "high")[i % 3])
        lines.append(HC.damage(rng, ln) if i % 4 == 3 else ln)
    lines += ["", " ", "\x00", "\xff"]
    data, offsets, omid, ocaps = answers(orc, lines)
    assert 2 * int((omid >= 0).sum()) > len(lines)
    check_hop_kernels(gorp, lines, data, offsets, omid, ocaps, kernels=(AUTO, HOPS, HOP_SLICES), compact=True)
    # terminated text, the terminators stripped by the kernels
    raw, off, want_lines = _terminated(rng, lines[:1000])
    td, to, tm, tc = answers(orc, want_lines)
    check_hop_kernels(gorp, want_lines, np.frombuffer(raw, np.uint8), off, tm, tc, strip_eol=True)
    # lines of 50-2000 bytes, announced as uneven: the hop slice kernel's pieces and rounds
    long_lines, tries = [], 0
    while len(long_lines) < 600 and tries < 20000:
        tries += 1
        ln = makers[rng.randrange(n_ext)](rng, style=("lower", "mixed", "high")[tries % 3], stretch=rng.choice([60, 300, 900]))
        if 50 <= len(ln) <= 2000:
            long_lines.append(HC.damage(rng, ln) if len(long_lines) % 5 == 4 else ln)
    assert len(long_lines) == 600 and max(len(ln) for ln in long_lines) > 1000
    ld, lo, lm, lc = answers(orc, long_lines)
    assert 2 * int((lm >= 0).sum()) > len(long_lines)
    check_hop_kernels(gorp, long_lines, ld, lo, lm, lc, kernels=(AUTO, HOP_SLICES), compact=True, uneven=2)
    assert gorp.stat(25) == HOP_SLICES
    # UTF-16 through the tile kernel: a unit above 0xFF inside a value of every third line that matched (U+0161's low byte is 'a')
    wide, n_wide = [], 0
    for i, ln in enumerate(lines[:900]):
        if i % 3 == 0 and omid[i] >= 0 and ocaps[i, 0] >= 0:
            g = rng.choice([g for g in range(gorp.max_groups) if ocaps[i, 2 * g] >= 0])
            at = int(ocaps[i, 2 * g] + ocaps[i, 2 * g + 1]) // 2
            ln = ln[:at] + rng.choice(["š", "中"]) + ln[at:]
            n_wide += 1
        wide.append(ln)
    assert n_wide > 100
    units, uoff = HC.utf16_csr(wide)
    wm, wc = HC.oracle_rows(orc, wide, gorp.max_groups)
    with_unit = np.array([any(ord(ch) > 0xFF for ch in ln) for ln in wide])
    assert int((wm[with_unit] >= 0).sum()) > 10 and int((wm[with_unit] < 0).sum()) > 10     # values whose class takes the unit, and others
    mid, caps = gorp.extract_batch(units, uoff, kernel=HOPS, uneven=1)
    assert gorp.stat(25) == HOPS
    assert_rows("UTF-16, tile kernel", wide, mid, caps, wm, wc)
    mo, _ = gorp.extract_batch(units, uoff, kernel=HOPS, uneven=1, match_only=True)
    assert gorp.stat(25) == HOPS
    assert_rows("UTF-16, tile kernel, match only", wide, mo, None, match_only_ids(wm), None)


def test_cut_lines_next_to_what_they_were_cut_from():
    """The run's window, the chain's eight bytes and the second chances all read past the lane's line end and rely on clamps (n <= e - p,
    qk <= e_chain twice, nu <= e - q).  Lines cut at random are followed by bytes that almost never continue the automaton's path, so
    a missing clamp still compared equal.  Here every cut of every base line is in the batch as line[:c] followed by line[c:]: behind
    the cut line's end lie exactly the bytes it was cut from.  A walk that runs over the end reports a match, or an offset beyond the
    cut; the oracle says what line[:c] is (mostly no match; a match when the cut falls inside the last value).  Lower-case and mixed
    base lines (mixed: the cuts fall inside second chances and tail retries), both hop kernels, captures and match only, and the
    tile kernel again on UTF-16."""
    rng = random.Random(31)
    syslog, meta = W.syslog_definition(64, seed=3)
    base_syslog = []
    for seed, mixed in ((5, False), (6, True)):
        d, o, _ = W.syslog_lines(meta, 20, seed=seed, line_bytes=100, corrupt_frac=0.0, mixed_case=mixed)
        base_syslog += [bytes(d[o[i]:o[i + 1]]).decode("latin-1") for i in range(20)]
    fielded, makers, frng = HC.fielded(48, 1)
    base_fielded = [makers[frng.randrange(48)](frng, style=style) for style in ("lower", "mixed") for _ in range(20)]
    for name, rules, flags, base in (("syslog", syslog, 0, base_syslog), ("fielded", fielded, N.GX_CREATE_TIER_HOP, base_fielded)):
        gorp, orc = Gorp.construct(rules, flags=flags), oracle_for(rules)
        assert gorp.stat(14) > 0 and gorp.stat(16) == gorp.stat(15)
        lines = [piece for ln in base for piece in HC.cut_pairs(ln)]
        assert 2000 < len(lines) < 20000
        data, offsets, omid, ocaps = answers(orc, lines)
        whole = {ln for ln in base}
        cut = np.array([i % 2 == 0 and lines[i] not in whole for i in range(len(lines))])
        # the oracle on the cut lines: most do not match, those cut inside the last value do
        assert 2 * int((omid[cut] < 0).sum()) > int(cut.sum()) and int((omid[cut] >= 0).sum()) > len(base), name
        assert int((omid[[i for i in range(len(lines)) if lines[i] in whole]] >= 0).sum()) >= len(base)   # (the base lines are well formed)
        check_hop_kernels(gorp, lines, data, offsets, omid, ocaps)
        units, uoff = HC.utf16_csr(lines)
        mid, caps = gorp.extract_batch(units, uoff, kernel=HOPS, uneven=1)
        assert gorp.stat(25) == HOPS
        assert_rows(name + ", UTF-16, tile kernel", lines, mid, caps, omid, ocaps)
        mo, _ = gorp.extract_batch(units, uoff, kernel=HOPS, uneven=1, match_only=True)
        assert gorp.stat(25) == HOPS
        assert_rows(name + ", UTF-16, tile kernel, match only", lines, mo, None, match_only_ids(omid), None)


def _device_batch(gorp, d, o, n, kernel, hint, match_only=False, compact=False, uneven=1):
    """One launch on device buffers; the results as torch tensors: (ids, offsets), ids alone for match only, the u16 rows for compact."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    width = 2 * gorp.max_groups
    if compact:
        rows = torch.empty((n, 1 + width), dtype=torch.int16, device="cuda")
        over = torch.zeros(1, dtype=torch.int64, device="cuda")
        gorp.extract_batch_device(d.data_ptr(), o.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=hint, kernel=kernel, compact=True,
                                  overflow_ptr=over.data_ptr(), uneven=uneven)
        torch.cuda.synchronize()
        assert gorp.stat(25) == kernel and int(over.item()) == 0
        return rows
    mid = torch.empty(n, dtype=torch.int32, device="cuda")
    caps = None if match_only else torch.empty((n, width), dtype=torch.int32, device="cuda")
    gorp.extract_batch_device(d.data_ptr(), o.data_ptr(), n, mid.data_ptr(), None if match_only else caps.data_ptr(), stream=st, line_bytes_hint=hint,
                              kernel=kernel, match_only=match_only, uneven=uneven)
    torch.cuda.synchronize()
    assert gorp.stat(25) == kernel
    return mid if match_only else (mid, caps)


def test_runs_of_every_length_at_every_window_offset():
    """A run's window is four aligned dwords from the lane's position: 16 - (p & 3) bytes.  Values of 0..40 bytes -- shorter than a
    window, filling one exactly, ending at a window's end, spanning three -- that begin at every address mod 4, for a state with a
    single interval (\\d+), with a loop set (\\w+: lower case alone, and mixed) and with a class that admits bytes above 0x7F (\\S+: ASCII
    alone, and with such a byte); the value followed by the line's end, by a separator and more text, or by a byte outside its class.
    The tile kernel stages a line at its buffer address mod 16 (gx_tile_body.hpp: make_round's skew), so on a 16-byte aligned device
    buffer the address of a value in the staging area mod 4 is its offset in the batch mod 4: the test lays the lines out so that every
    (address mod 4, length) occurs for every kind, and asserts that table from the offsets."""
    import torch
    rng = random.Random(17)
    kinds = {"d": ("\\d+", ";", "x"), "w": ("\\w+", ";", "-"), "s": ("\\S+", " ", " ")}       # pattern, separator, a byte outside the class
    rules = []
    for letter, (rx, sep, _) in kinds.items():
        value = ["extractor", "v", [["pattern", rx]]]
        rules.append(FlattenedExtraction("ends_" + letter, [["text", letter], ["pattern", "p+"], ["text", "="], value]))
        rules.append(FlattenedExtraction("more_" + letter, [["text", letter.upper()], ["pattern", "p+"], ["text", "="], value, ["text", sep],
                                                            ["extractor", "t", [["pattern", "\\w+"]]]]))
    gorp, orc = Gorp.construct(rules, flags=N.GX_CREATE_TIER_HOP), oracle_for(rules)
    assert gorp.stat(14) > 0 and gorp.stat(16) == gorp.stat(15)
    alphabets = [("d", HC.DIGITS, ""), ("w", HC.LOWER, ""), ("w", HC.LOWER + HC.UPPER + HC.DIGITS + "_", ""), ("s", HC.LOWER + "/?.:-", ""),
                 ("s", HC.LOWER + "/?.:-", "\xe9\xff")]
    lines, cells, at = [], {}, 0
    for a, (letter, alphabet, high) in enumerate(alphabets):
        rx, sep, outside = kinds[letter]
        for follow in ("end", "more", "outside"):
            for length in range(41):
                for residue in range(4):
                    pre = 1 + (residue - (at + 3)) % 4          # "<letter>" + pre * "p" + "=": the value begins at at + pre + 2
                    v = [rng.choice(alphabet) for _ in range(length)]
                    if high and length:
                        v[rng.randrange(length)] = rng.choice(high)
                    head = (letter.upper() if follow == "more" else letter) + "p" * pre + "="
                    ln = head + "".join(v) + {"end": "", "more": sep + "tail9", "outside": outside}[follow]
                    cells.setdefault((a, follow), set()).add(((at + len(head)) % 4, length))
                    lines.append(ln)
                    at += len(ln)
    data, offsets, omid, ocaps = answers(orc, lines)
    for key, have in cells.items():
        assert have == {(r, n) for r in range(4) for n in range(41)}, key
    # ... and the same table from the oracle's offsets, for the lines that match (every length but 0, "end" and "more")
    begins = offsets[:-1].astype(np.int64) + ocaps[:, 0]
    seen = {(int(b % 4), int(e - s)) for b, s, e, m in zip(begins, ocaps[:, 0], ocaps[:, 1], omid) if m >= 0}
    assert seen == {(r, n) for r in range(4) for n in range(1, 41)}
    assert int((omid >= 0).sum()) >= len(alphabets) * 2 * 40 * 4
    d, o = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda().to(torch.uint32)
    assert d.data_ptr() % 16 == 0
    for kernel in (HOPS, HOP_SLICES):
        mid, caps = _device_batch(gorp, d, o, len(lines), kernel, 32)
        assert_rows("kernel %d" % kernel, lines, mid.cpu().numpy(), caps.cpu().numpy(), omid, ocaps)
        mo = _device_batch(gorp, d, o, len(lines), kernel, 32, match_only=True)
        assert_rows("kernel %d, match only" % kernel, lines, mo.cpu().numpy(), None, match_only_ids(omid), None)
    check_hop_kernels(gorp, lines, data, offsets, omid, ocaps, compact=True)


SAMPLE_TILES = 61      # a prime: no grid of the tile kernel (CUs x 1..12 workgroups, 3 072 at most) is a multiple of it on a device of < 61 x 61 CUs


def _alternating_sample(rng, lower, mixed):
    """SAMPLE_TILES tiles: blocks of 1-4 tiles (64-256 lines) of lower-case lines and of mixed lines in turn, one line in twenty damaged.
    Returns the lines and each tile's kind (0 lower case, 1 mixed)."""
    lines, kinds, pools, blk = [], [], (iter(lower), iter(mixed)), 0
    while len(kinds) < SAMPLE_TILES:
        for _ in range(min(rng.randint(1, 4), SAMPLE_TILES - len(kinds))):
            kinds.append(blk % 2)
            for _ in range(64):
                ln = next(pools[blk % 2])
                lines.append(HC.damage(rng, ln) if rng.random() < 0.05 else ln)
        blk += 1
    return lines, kinds


def _kind_changes(kinds, shift):
    """Of the tiles t of a batch that repeats the sample, how many are lower case while tile t + shift is mixed (as many are mixed while
    tile t + shift is lower case: the sample is a cycle)."""
    T = len(kinds)
    return sum(kinds[t] == 0 and kinds[(t + shift) % T] == 1 for t in range(T))


def test_tile_walk_enters_and_leaves_second_chance_mode():
    """The tile kernel compiles its all-hot walk twice: without the second chances (loop sets, tail sets), where a lane that wanted one
    takes its exact step and the wave notes it, and with them -- for the tile the SAME WAVE walks next, and back again after a tile
    that needed none (gx_hop_dev.hpp: walk_hop; gx_tile_body.hpp: hop_second starts false for every wave).  launch_extract_tile
    launches at most ceil(tiles / waves per workgroup) workgroups, so in a batch with fewer tiles than the device holds waves every
    wave walks one tile and the walk with second chances never runs: the suite's mixed-case batches were 20 000 and 6 000 lines, 313
    and 94 tiles, and only the full-size benchmark reached that code.

    The grid arithmetic this test rests on (the product build has no counter for the mode, and none is to be added): the launch has
    `grid` = CUs x blocks_per_cu workgroups (3 072 at most) of `nwaves` waves with blocks_per_cu x nwaves <= 16 waves per CU; a tile is
    64 lines.  With n >= 4 x 64 x 16 x CUs lines (1 048 576 on 256 CUs) there are four tiles for every wave the grid can hold.  The
    first two tiles of every wave are fixed, tile_at(wg, wave) and tile_at(wg, nwaves + wave) with tile_at(wg, k) = wg + k x grid: a
    wave's second tile lies nwaves x grid tiles behind its first, and its later ones, drawn from the workgroup's counter, a multiple
    of grid behind that.  So every wave walks at least two tiles, four on average, and which KIND of tile follows which is decided
    by the sample's tiles modulo its length.  The sample is SAMPLE_TILES = 61 tiles, a prime that divides no grid and no nwaves x
    grid (asserted: it does not divide the CU count; blocks_per_cu <= 12 and nwaves <= 16 are smaller), in blocks of 1-4 tiles of
    lower-case lines (no second chance wanted: the mode is left) and of mixed lines (wanted: the mode is entered) in turn; and the
    test asserts on the host that at EVERY shift that is no multiple of 61 at least an eighth of the tiles are lower case with a
    mixed tile that far behind, and as many the other way round.  Whatever the grid, both transitions happen all over it, for each
    definition, in every row form (with u16 rows and match only no tile is taken from another workgroup: the fixed shifts are all
    there is).  Every copy of the sample must equal the oracle's answer for the WHOLE sample: captures as dense and as u16 rows, and
    match only.

    A limit: the all-hot precondition (gx_stat 16 == 15) is known for the fused automaton's image only.  The match-only launches walk
    the match automaton's image (gx_stat 22), whose reachable count no stat exposes (gx_stat 23 is its hot count): for them the test
    cannot tell whether the walk with second chances ran, or the walk that keeps records (which always carries them)."""
    import torch
    rng = random.Random(59)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_min = 4 * 64 * 16 * cus
    syslog, meta = W.syslog_definition(64, seed=3)
    pools = []
    for mixed in (False, True):
        d, o, _ = W.syslog_lines(meta, 64 * SAMPLE_TILES, seed=61 + mixed, corrupt_frac=0.0, mixed_case=mixed)
        pools.append([bytes(d[o[i]:o[i + 1]]).decode("latin-1") for i in range(64 * SAMPLE_TILES)])
    fielded, makers, frng = HC.fielded(48, 1)
    fpools = [[makers[frng.randrange(48)](frng, style=style) for _ in range(64 * SAMPLE_TILES)] for style in ("lower", "mixed")]
    for name, rules, flags, (lower, mixed) in (("syslog", syslog, 0, pools), ("fielded", fielded, N.GX_CREATE_TIER_HOP, fpools)):
        gorp, orc = Gorp.construct(rules, flags=flags), oracle_for(rules)
        assert gorp.stat(14) > 0 and gorp.stat(16) == gorp.stat(15), name       # every reachable record in LDS: the all-hot walk, both modes
        assert 0 < gorp.stat(18) <= 16                                          # waves per workgroup
        lines, kinds = _alternating_sample(rng, lower, mixed)
        base_n = len(lines)
        assert base_n == 64 * SAMPLE_TILES and cus % SAMPLE_TILES != 0 and 3072 % SAMPLE_TILES != 0
        changes = [_kind_changes(kinds, shift) for shift in range(1, SAMPLE_TILES)]
        assert 8 * min(changes) >= SAMPLE_TILES, (name, changes)     # both transitions at every shift a grid can make
        data, offsets, omid, ocaps = answers(orc, lines)
        assert 2 * int((omid >= 0).sum()) > base_n
        reps = (n_min + base_n - 1) // base_n
        n = reps * base_n
        assert n >= n_min
        hint = int(offsets[-1]) // base_n + 1
        d, o = _tiled_on_device(data, offsets, reps)
        width = 2 * gorp.max_groups
        want_id, want_caps = torch.from_numpy(omid).cuda(), torch.from_numpy(ocaps).cuda()

        def first_bad(bad):      # the first line of the sample that differs in any copy
            i = int(torch.nonzero(bad.view(reps, base_n).any(dim=0))[0, 0])
            return "%s: %d lines differ; first: line %d of the sample, %r" % (name, int(bad.sum()), i, lines[i])

        mid, caps = _device_batch(gorp, d, o, n, HOPS, hint)
        bad = (mid.view(reps, base_n) != want_id[None, :]) | (caps.view(reps, base_n, width) != want_caps[None, :, :]).any(dim=2)
        assert not bool(bad.any()), first_bad(bad)
        rows = _device_batch(gorp, d, o, n, HOPS, hint, compact=True).to(torch.int32).view(reps, base_n, 1 + width)   # (-1 stays -1 through int16; offsets < 32 768)
        bad = (rows[:, :, 0] != want_id[None, :]) | (rows[:, :, 1:] != want_caps[None, :, :]).any(dim=2)
        assert not bool(bad.any()), first_bad(bad)
        del rows, caps
        mo = _device_batch(gorp, d, o, n, HOPS, hint, match_only=True)
        bad = mo.view(reps, base_n) != torch.from_numpy(match_only_ids(omid)).cuda()[None, :]
        assert not bool(bad.any()), first_bad(bad)
