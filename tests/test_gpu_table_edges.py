"""The batch kernels on table images at the limits of their formats (tests/table_edge_cases.py): 250-253 character classes, dense rows
that fill the 16-bit LDS address space, range records at their LDS budget, range records whose successors need more than 16 bits,
match states beyond 2^15 and the two-pass layout a definition without a fused automaton gets.  Every comparison is bit-exact
against the oracle; every launch asserts through gx_stat 25 which kernel ran, over every kernel the handle can take.
tests/test_table_edges_host.py pins on the CPU which image each case has.

For the syslog cases each test first asserts, with the oracle alone, that every extraction wins at least one line: these automata
are numbered by depth, so a fully matched line walks the highest-numbered states -- the top of each table is read."""
import ctypes as C

import numpy as np
import pytest

import hop_cases as HC
import table_edge_cases as TE
from blob_interp import Blob
from gorp_amd import _native as N
from gorp_amd import gorp as G
from gorp_amd.gorp import Gorp
from test_gpu_hop import assert_rows, match_only_ids
from test_gpu_parity import oracle_for

pytestmark = pytest.mark.gpu

AUTO, TILES, SLICES, PER_LINE, LANES = N.GX_KERNEL_AUTO, N.GX_KERNEL_TILES, N.GX_KERNEL_SLICES, N.GX_KERNEL_PER_LINE, N.GX_KERNEL_LANES
HOPS, HOP_SLICES = N.GX_KERNEL_HOPS, N.GX_KERNEL_HOP_SLICES
NAMED = (TILES, SLICES, LANES, PER_LINE, HOPS, HOP_SLICES)


def takes(gorp, kernel, mo):
    """Whether a batch that names `kernel` runs on it (gx_images.cpp: plan_batch), from the handle's own statistics: the tile kernel
    needs a table image and room for four waves beside it (6: its waves); the slice kernel walks the fused automaton (39); the lane
    kernel does for captures (10 / 11: its waves); the hop kernels need the hop tables of the batch's kind (18, 19 / 22); the
    per-line kernel takes everything.  A kernel the handle cannot take is not asked for: the batch would fall through to another."""
    if kernel == TILES:
        return gorp.stat(6) > 0
    if kernel == SLICES:
        return gorp.stat(7) != 0 and gorp.stat(39) == 1
    if kernel == LANES:
        return gorp.stat(11 if mo else 10) > 0
    if kernel == HOPS:
        return gorp.stat(22 if mo else 18) > 0
    if kernel == HOP_SLICES:
        return gorp.stat(22 if mo else 19) > 0
    return True


def ran(gorp, kernel, mo):
    """The launch took the kernel it named; left to itself, one of those the handle can take."""
    got = gorp.stat(25)
    if kernel == AUTO:
        assert got in [k for k in NAMED if takes(gorp, k, mo)], (got, mo)
    else:
        assert got == kernel, (kernel, got, mo)


class _Lines:
    """line i of a batch, for assert_rows' message"""

    def __init__(self, data, offsets):
        self.data, self.offsets = data, offsets

    def __getitem__(self, i):
        return bytes(self.data[int(self.offsets[i]):int(self.offsets[i + 1])])


def check_kernel(gorp, kernel, batch, what, forms=(0, 1, 2), **kw):
    """One batch through one kernel: captures as dense rows (form 0), u16 rows (1) and u8 rows (2: up to 126 extractions), and match
    only; each launch must have run the kernel.  An offset a compact row cannot hold is clipped and counted, none where the
    oracle's offsets all fit (overflow == 0)."""
    data, offsets, omid, ocaps = batch
    lines = _Lines(data, offsets)
    if takes(gorp, kernel, False):
        for form in forms:
            tag = "%s, kernel %d, rows %d" % (what, kernel, form)
            if form == 0:
                mid, caps = gorp.extract_batch(data, offsets, kernel=kernel, **kw)
                ran(gorp, kernel, False)
                assert_rows(tag, lines, mid, caps, omid, ocaps)
                continue
            if form == 2 and len(gorp.getExtractions()) > 126:
                continue
            limit = 65534 if form == 1 else 254
            rows, over = gorp.extract_batch(data, offsets, kernel=kernel, compact=form, **kw)
            ran(gorp, kernel, False)
            cm, cc = G.unpack_rows(rows)
            big = ocaps > limit
            assert over == int(big.sum()), (tag, over, int(big.sum()))
            assert_rows(tag, lines, cm, cc, omid, np.where(big, limit, ocaps))
    if takes(gorp, kernel, True):
        mo, _ = gorp.extract_batch(data, offsets, kernel=kernel, match_only=True, **kw)
        ran(gorp, kernel, True)
        assert_rows("%s, kernel %d, match only" % (what, kernel), lines, mo, None, match_only_ids(omid), None)


def check_every_kernel(gorp, batch, what, forms=(0, 1, 2), kernels=(AUTO,) + NAMED, **kw):
    for kernel in kernels:
        check_kernel(gorp, kernel, batch, what, forms, **kw)


def blob_final_states(blob, data, offsets):
    """The state of the product's own match automaton every line ends in (blob_interp.Blob.match_state, all lines at once)."""
    cls = blob.cls256[np.asarray(data)].astype(np.int64)
    pos, end = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
    st = np.zeros(len(pos), np.int64)
    idx = np.nonzero(pos < end)[0]
    while len(idx):
        st[idx] = blob.m_next[st[idx], cls[pos[idx]]]
        pos[idx] += 1
        idx = idx[pos[idx] < end[idx]]
    return st


def check_match_batch(gorp, orc, batch, what):
    """gx_match_batch: the first accepting extraction of every line against the oracle; the final states -- a dense row is a state, so
    the tile kernel gives them where the match-only tables are dense rows, the per-line kernel elsewhere -- against a walk of the
    product's own tables on the host (equal outright for every line that does not end in the dead state), and what
    gx_state_accepts reads off them against the oracle's PolyMatcher.match on a sample.  Returns the states."""
    data, offsets, omid, _ = batch
    n = len(offsets) - 1
    first, states = np.zeros(n, np.int32), np.zeros(n, np.int32)
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    G._check(N.lib().gx_match_batch(gorp._h.ptr, data.ctypes.data, offsets.ctypes.data, n, first.ctypes.data, states.ctypes.data, C.byref(o)))
    assert gorp.stat(25) == (TILES if gorp.stat(9) in (1, 2) else PER_LINE), (what, gorp.stat(25), gorp.stat(9))
    lines = _Lines(data, offsets)
    assert_rows(what + ", gx_match_batch", lines, first, None, match_only_ids(omid), None)
    blob = Blob(gorp.blob())
    want = blob_final_states(blob, data, offsets)
    live = want != blob.m_dead
    assert np.array_equal(states[live], want[live]), (what, int((states[live] != want[live]).sum()))
    cap = max(1, gorp.num_extractions)
    buf = np.zeros(cap, np.int32)

    def accepts(st):
        c = N.lib().gx_state_accepts(gorp._h.ptr, int(st), buf.ctypes.data, cap)
        return buf[:c].tolist()

    for st in np.unique(states[~live]).tolist():
        assert accepts(st) == [], (what, st)
    for i in list(range(0, n, max(1, n // 64))) + [int(np.argmax(states))]:
        assert accepts(states[i]) == orc.match(lines[i].decode("latin-1")), (what, i, lines[i][:60])
    return states


@pytest.fixture(scope="module")
def edge():
    """Every definition, oracle, handle and batch of the module, built once."""
    cache = {}

    class Edge:
        def made(self, key, make):
            if key not in cache:
                cache[key] = make()
            return cache[key]

        def definition(self, name):
            return self.made(("definition", name), lambda: TE.definition(name))

        def oracle(self, name):
            return self.made(("oracle", name), lambda: oracle_for(self.definition(name)[0]))

        def gorp(self, name, flags):
            """The handle, its tables asserted to be what table_edge_cases.EXPECT says."""
            def make():
                g = Gorp.construct(self.definition(name)[0], flags=flags)
                TE.expected(g, name, flags)
                return g
            return self.made(("gorp", name, flags), make)

        def batch(self, name, n_lines, lengths=None):
            """(data, offsets, the oracle's ids, the oracle's offsets): literal_lines for the class cases; for the syslog cases lines of
            200 bytes, or of lengths[0]..lengths[1] bytes, one in ten damaged.  An even syslog batch must let every extraction win."""
            def make():
                rules, meta = self.definition(name)
                if meta is None:
                    data, offsets = G.lines_to_csr(TE.literal_lines(len(rules), n_lines))
                else:
                    data, offsets = TE.syslog_batch(meta, n_lines, seed=len(rules) + (1 if lengths else 0), lengths=lengths)
                omid, ocaps = self.oracle(name).extract_batch(data, offsets, nthreads=8)
                if meta is not None and lengths is None:
                    assert n_lines >= 20 * len(rules)
                    wins = np.bincount(omid[omid >= 0], minlength=len(rules))
                    assert int(wins.min()) >= 1, (name, int((wins == 0).sum()))
                    assert int(ocaps.max()) <= 254       # (every offset fits a u8 row: overflow == 0 is what check_kernel asserts)
                if meta is not None:
                    assert 4 * int((omid >= 0).sum()) > 3 * n_lines and int((omid < 0).sum()) > n_lines // 50, name
                return data, offsets, omid, ocaps
            return self.made(("batch", name, n_lines, lengths), make)

    yield Edge()
    cache.clear()


# ---- character classes -------------------------------------------------------------------------------------------------------
CLASS_CASES = [(n, f) for n in (250, 251, 252, 253) for f in (0, TE.L2, TE.REC, TE.RECG)] + [(253, TE.PROGRAMS)]


@pytest.mark.parametrize("n,flags", CLASS_CASES)
def test_class_ids_up_to_the_limit(edge, n, flags):
    """250 classes are the most range records take, 252 the most any table image takes (a column offset, class * 4, is a 10-bit field
    with three more columns behind it); with 253 the per-line kernel is all there is -- on the automata, and with GX_CREATE_PROGRAMS on
    the extractions' programs, whose class sets are 256 bits.  Every literal byte heads some line, so every class id is looked up
    and every column of the start state's row is read; at least one match belongs to an extraction numbered 240 or above."""
    name = "classes%d" % n
    gorp, orc = edge.gorp(name, flags), edge.oracle(name)
    batch = edge.batch(name, 3000)
    omid = batch[2]
    assert int((omid >= 0).sum()) >= 300 and int(omid.max()) >= 240
    if flags == TE.PROGRAMS:
        assert gorp.stat(27) == n
    if n == 253:
        assert [k for k in NAMED if takes(gorp, k, False) or takes(gorp, k, True)] == [PER_LINE]
    check_every_kernel(gorp, batch, "%d classes, flags %d" % (n, flags))
    check_match_batch(gorp, orc, batch, "%d classes, flags %d" % (n, flags))


# ---- dense rows in LDS at 62 KB ----------------------------------------------------------------------------------------------
DENSE = ["dense_1x13", "dense_1x14", "dense_2x6", "dense_2x7"]


def _with_wide_units(batch):
    """The batch's lines as str, with U+4E2D in place of one character of every seventh (at 13 i mod the length in line i: inside
    literals, numbers, words and \\S+ values in turn)."""
    data, offsets = batch[0], batch[1]
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]).decode("latin-1") for i in range(len(offsets) - 1)]
    return [ln[:13 * i % len(ln)] + "中" + ln[13 * i % len(ln) + 1:] if i % 7 == 0 else ln for i, ln in enumerate(lines)]


@pytest.mark.parametrize("name", DENSE)
def test_dense_rows_filling_lds_addresses(edge, name):
    """Two definitions whose dense rows end just below LDS address 65 536 (images of 62 448 and 61 584 bytes: successors at and above
    0x8000 in every row of the deeper half) and their neighbours of one key more, which leave LDS for range records and hop tables.
    4 000 lines announced as 50, 200 and 2 000 bytes long, as even and as uneven; every kernel the handle can take in every row
    form; gx_match_batch's states; and the lines as UTF-16 with a unit above 0xFF in every seventh -- the tile kernel's build that
    reads code units (13 KB of staging, 8 waves at most), or the hop tier's where the rows left LDS."""
    gorp, orc = edge.gorp(name, 0), edge.oracle(name)
    batch = edge.batch(name, 4000)
    check_every_kernel(gorp, batch, name, line_bytes_hint=200)
    for hint in (50, 200, 2000):
        for uneven in (1, 2):
            check_kernel(gorp, AUTO, batch, "%s, hint %d, uneven %d" % (name, hint, uneven), forms=(0, 1), line_bytes_hint=hint, uneven=uneven)
            if gorp.stat(7) == 1 and hint <= 255 and uneven == 1:
                assert gorp.stat(25) == TILES
    check_match_batch(gorp, orc, batch, name)
    wide = _with_wide_units(batch)
    units, uoff = HC.utf16_csr(wide)
    wm, wc = HC.oracle_rows(orc, wide, gorp.max_groups)
    with_unit = np.array([i % 7 == 0 for i in range(len(wide))])
    assert int((wm[with_unit] >= 0).sum()) > 50 and int((wm[with_unit] < 0).sum()) > 50     # (\S+ takes the unit, \d+ and \w+ do not)
    mid, caps = gorp.extract_batch(units, uoff, line_bytes_hint=200, uneven=1)
    assert gorp.stat(25) == (TILES if gorp.stat(7) == 1 else HOPS)
    assert_rows(name + ", UTF-16", wide, mid, caps, wm, wc)
    mo, _ = gorp.extract_batch(units, uoff, line_bytes_hint=200, uneven=1, match_only=True)
    assert gorp.stat(25) == (TILES if gorp.stat(7) == 1 else HOPS)
    assert_rows(name + ", UTF-16, match only", wide, mo, None, match_only_ids(wm), None)


@pytest.mark.parametrize("name", DENSE)
def test_dense_rows_without_the_fused_automaton(edge, name):
    """GX_CREATE_NO_FUSED on the same four: the two-pass layout, whose rows (the match automaton's and one capture automaton per
    extraction) fit LDS for all of them -- the tier is in table_edge_cases.EXPECT."""
    gorp = edge.gorp(name, TE.NO_FUSED)
    assert gorp.stat(39) == 0
    check_every_kernel(gorp, edge.batch(name, 4000), name + ", no fused automaton", line_bytes_hint=200)


@pytest.mark.parametrize("name", DENSE)
def test_dense_rows_under_the_resident_wave(edge, name):
    """GX_CREATE_RESIDENT_ONE: 200 single lines answered by the resident wave, which copies the whole 62 KB image into LDS, against
    the launch-per-call handle and the oracle.  Where the rows are not in LDS the handle has no such wave (gx_stat 28 == -1) and the
    calls take the usual path."""
    plain, resident, orc = edge.gorp(name, 0), edge.gorp(name, TE.RESIDENT), edge.oracle(name)
    data, offsets = edge.batch(name, 4000)[:2]
    assert plain.stat(28) == -1
    hits = 0
    for i in range(200):
        ln = bytes(data[int(offsets[i]):int(offsets[i + 1])]).decode("latin-1")
        want = orc.extract(ln)
        a, b = plain.extractSafe(ln), resident.extractSafe(ln)
        assert (a is None) == (b is None) == (want[0] < 0), (i, ln)
        if a is not None:
            hits += 1
            assert a.getId() == b.getId() == "rule%d" % want[0], (i, ln)
            assert b._extractedValues == a._extractedValues == [None if g is None else ln[g[0]:g[1]] for g in want[1]], (i, ln)
    assert hits > 150
    if resident.stat(7) == 1:
        assert resident.stat(28) >= 1
    else:
        assert resident.stat(28) == -1


# ---- range records at the LDS budget -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [80, 96])
def test_range_records_at_the_lds_budget(edge, n):
    """80 extractions: an image of 97 040 bytes of range records, within 1 300 bytes of the 96 KB that may stay in LDS -- no definition
    leaves the waves less room beside its tables; 96 extractions: the same records in global memory.  6 000 lines of 200 bytes
    announced as 200 and as 2 000 bytes long, and 3 000 lines of 50-2 000 bytes."""
    name = "records%d" % n
    gorp = edge.gorp(name, TE.REC)
    assert (gorp.stat(12) > 90 * 1024) == (n == 80) and gorp.stat(36) > 0
    even = edge.batch(name, 6000)
    check_every_kernel(gorp, even, name, line_bytes_hint=200)
    check_kernel(gorp, AUTO, even, name + ", hint 2000", forms=(0, 1), line_bytes_hint=2000)
    mixed = edge.batch(name, 3000, lengths=(50, 2000))
    check_every_kernel(gorp, mixed, name + ", 50-2000 bytes", kernels=(AUTO, SLICES, LANES), uneven=2)


# ---- range records with successors beyond 16 bits ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide440", "wide_max"])
def test_range_records_with_wide_successors(edge, name):
    """Range records in global memory carry 22-bit successors because two automata of up to 65 536 states take more than 65 535
    records together.  The largest definition that has them (table_edge_cases.WIDE_MAX extractions) has 68 218 for capture batches
    (gx_stat 36): successors with bit 16 set, on the path of every line of the later-numbered states.  440 extractions have
    58 089: the most the syslog family gives below 2^16, every successor's upper byte full.  Every extraction wins a line."""
    gorp = edge.gorp(name, TE.RECG)
    n = len(edge.definition(name)[0])
    if name == "wide_max":
        assert gorp.stat(36) > 65535
    else:
        assert 0xE000 < gorp.stat(36) <= 65535
    assert 0 < gorp.stat(37) <= 65535      # (the match automaton's own image stays within 16 bits at both sizes)
    check_every_kernel(gorp, edge.batch(name, 20 * n), name, forms=(0, 1), line_bytes_hint=200)
    check_every_kernel(gorp, edge.batch(name, 5 * n, lengths=(50, 2000)), name + ", 50-2000 bytes", forms=(0, 1), kernels=(AUTO, SLICES, LANES), uneven=2)


# ---- match states beyond 2^15, no fused automaton ----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, TE.L2])
def test_match_states_beyond_15_bits(edge, flags):
    """570 extractions: 33 282 states of the match automaton -- a state index is 16 bits of a dense entry, and of a hop record -- and
    no fused automaton, so capture batches take the two-pass layout on rows in global memory: what every definition beyond about
    520 extractions gets, and what the suite had only under GX_CREATE_NO_FUSED on small ones.  Match-only batches have the hop
    tier of the match automaton alone (not under GX_CREATE_TIER_L2).  gx_match_batch returns final states at and above 32 768."""
    name = "states570"
    gorp, orc = edge.gorp(name, flags), edge.oracle(name)
    assert gorp.stat(0) > 32768 and gorp.stat(39) == 0
    assert (gorp.stat(22) == gorp.stat(0)) == (flags == 0)
    even = edge.batch(name, 12000)
    check_every_kernel(gorp, even, "570 extractions, flags %d" % flags, forms=(0, 1), line_bytes_hint=200)
    if flags == 0:
        # (check_every_kernel ran match-only batches under AUTO, HOPS and HOP_SLICES; left to itself the batch takes a hop kernel)
        assert takes(gorp, HOPS, True) and takes(gorp, HOP_SLICES, True) and not takes(gorp, HOPS, False)
        mo, _ = gorp.extract_batch(even[0], even[1], match_only=True, line_bytes_hint=200)
        assert gorp.stat(25) == HOPS
        assert_rows("570 extractions, match only", _Lines(even[0], even[1]), mo, None, match_only_ids(even[2]), None)
    states = check_match_batch(gorp, orc, even, "570 extractions, flags %d" % flags)
    assert int(states.max()) >= 32768 and int((states >= 32768).sum()) > 100
    mixed = edge.batch(name, 6000, lengths=(50, 2000))
    check_every_kernel(gorp, mixed, "570 extractions, flags %d, 50-2000 bytes" % flags, forms=(0, 1), kernels=(AUTO, TILES, LANES, HOP_SLICES), uneven=2)
