"""The lines a batch kernel leaves to a second launch, against the CPU oracle bit for bit.

Every batch kernel answers most lines itself and leaves a few: the tile kernels a line that does not fit a wave's staging area
(length + skew + 48 <= stage_bytes, skew = 0..15 from the line's address), the lane and hop slice kernels a line longer than their
16-bit positions.  The follow-up kernel restates that rule to find those lines and the host restates it to decide whether a
caller's max_line_bytes promise lets it drop the follow-up launch.  If two of the three disagree by one byte at one alignment a
row is never written (the sentinel shows) or written twice (the overflow count of compact rows is too large).  The tests here put
every length at every alignment across that edge, in every result format, with and without promises -- and then break promises
on purpose (a documented, handled condition), alone and stacked on one stream.

Device buffers throughout: the promise exists only there.  Result buffers are filled with a sentinel before every launch."""
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import gorp as G
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp, lines_to_csr
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HEAD = "[1]: GET 5ms /"
SHORT = "[2]: PUT 1ms /y"
ROW_LIMIT = {1: 65534, 2: 254}          # the largest offset u16 rows and u8 rows hold
ENDS = ("\n", "\r\n", "\r")


def oracle_for(definition):
    built = [e.build() for e in definition]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


def readme_line(k):
    return HEAD + "x" * (k - len(HEAD))


def join_csr(parts):
    """(data, offsets) pairs of W.syslog_lines -> one CSR batch."""
    data = np.concatenate([p[0] for p in parts])
    lens = np.concatenate([np.diff(p[1].astype(np.int64)) for p in parts])
    offsets = np.zeros(len(lens) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(lens)
    return data, offsets


def first_difference(got_m, got_c, want_m, want_c, lens):
    bad = np.flatnonzero((got_m != want_m) | (got_c != want_c).any(axis=1))
    i = int(bad[0])
    return "%d of %d lines differ; first: line %d (%d units in memory): got id %d %s, oracle %d %s" % (
        len(bad), len(want_m), i, int(lens[i]), int(got_m[i]), got_c[i].tolist(), int(want_m[i]), want_c[i].tolist())


class DeviceBatch:
    """One CSR batch in device memory at a movable alignment, the oracle's answers for it, and launches of it in the three result
    formats (fmt 0: int32 match ids and offsets, 1: u16 rows, 2: u8 rows)."""

    def __init__(self, gorp, data, offsets, omid, ocaps, kernel=0, hint=0, strip_eol=False, utf16=False):
        import torch
        self.torch = torch
        self.gorp, self.kernel, self.hint, self.strip_eol, self.utf16 = gorp, kernel, hint, strip_eol, utf16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        self.lens = np.diff(self.offsets.astype(np.int64))
        self.n = len(self.lens)
        self.omid, self.ocaps = omid, ocaps
        assert len(omid) == self.n and ocaps.shape == (self.n, 2 * gorp.max_groups)
        self.src = torch.from_numpy(data).cuda()                       # the one upload
        self.buf = torch.zeros(len(data) + 64, dtype=self.src.dtype, device="cuda")
        self.o = torch.from_numpy(self.offsets).cuda()
        self.slots = 2 * gorp.max_groups
        self.out = {}
        self.place(0)

    def place(self, s):
        """The batch at `s` units past a 256-byte boundary."""
        assert self.buf.data_ptr() % 256 == 0
        self.buf[s:s + len(self.src)].copy_(self.src)
        self.ptr = self.buf.data_ptr() + s * self.src.element_size()
        self.shift = s

    def buffers(self, fmt, n=None):
        """Fresh result buffers full of sentinels and a zeroed overflow counter, as launch() returns them."""
        torch = self.torch
        n = self.n if n is None else n
        mid = torch.full((n,), -7, dtype=torch.int32, device="cuda") if fmt == 0 else None
        if fmt == 0:
            rows = torch.full((n, self.slots), -7, dtype=torch.int32, device="cuda")
        else:
            rows = torch.full((n, 1 + self.slots), 7, dtype=torch.int16 if fmt == 1 else torch.uint8, device="cuda")
        over = torch.zeros(1, dtype=torch.int64, device="cuda") if fmt else None
        torch.cuda.current_stream().synchronize()         # (the fills, before a launch on whichever stream)
        return fmt, n, mid, rows, over

    def launch(self, fmt, n=None, promise=0, no_sync=False, stream=None, offsets_ptr=None, into=None):
        """One launch into `into` (default: fresh buffers()).  Returns the buffers (still on the device)."""
        fmt, n, mid, rows, over = into or self.buffers(fmt, n)
        self.gorp.extract_batch_device(self.ptr, offsets_ptr or self.o.data_ptr(), n, mid.data_ptr() if fmt == 0 else None, rows.data_ptr(),
                                       stream=stream, no_sync=no_sync, strip_eol=self.strip_eol, line_bytes_hint=self.hint, kernel=self.kernel,
                                       compact=fmt, overflow_ptr=over.data_ptr() if fmt else None, max_line_bytes=promise, utf16=self.utf16)
        return fmt, n, mid, rows, over

    def read(self, launched):
        """-> (match ids, offsets, overflow count or None) on the host; the caller has waited for the launch."""
        fmt, n, mid, rows, over = launched
        if fmt == 0:
            return mid.cpu().numpy(), rows.cpu().numpy(), None
        m, c = G.unpack_rows(rows.cpu().numpy().view(np.uint16 if fmt == 1 else np.uint8))
        return m, c, int(over.item())

    def want(self, fmt, n=None, first=0):
        """The oracle's answers in the format's terms: offsets above the format's limit stored as the limit, and counted."""
        n = self.n - first if n is None else n
        m, c = self.omid[first:first + n], self.ocaps[first:first + n]
        if fmt == 0:
            return m, c, None
        big = c > ROW_LIMIT[fmt]
        return m, np.where(big, ROW_LIMIT[fmt], c), int(big.sum())

    def check_not_launched(self, launched, what):
        """A call that was refused at submission wrote nothing: every row still holds the sentinel, the counter is 0."""
        self.torch.cuda.synchronize()
        gm, gc, gover = self.read(launched)
        fill = -7 if launched[0] == 0 else 7
        assert (gm == fill).all() and (gc == fill).all() and not gover, what + ": refused at submission, yet rows were written"

    def check(self, launched, what, first=0):
        """Every line of the launch against the oracle, and the overflow count exactly."""
        self.torch.cuda.synchronize()
        fmt, n = launched[0], launched[1]
        gm, gc, gover = self.read(launched)
        wm, wc, wover = self.want(fmt, n, first)
        where = "%s, format %d, %d lines at alignment %d" % (what, fmt, n, self.shift)
        assert np.array_equal(gm, wm) and np.array_equal(gc, wc), where + ": " + first_difference(gm, gc, wm, wc, self.lens[first:first + n])
        assert gover == wover, "%s: overflow counter %s, the oracle has %s offsets above %d (a line answered twice, or never)" % (
            where, gover, wover, ROW_LIMIT.get(fmt, 0))


def edge_of(gorp, probe, kernel):
    """(fits, limit) of the plan a launch like `probe` gets: gx_stat(h, 31) and (h, 32) after one launch of it.  Used only to say
    where the dense part of a sweep goes and to prove that the sweep held the edge; every expected value is the oracle's."""
    probe.check(probe.launch(0), "probe")
    assert gorp.stat(25) == kernel
    fits, limit = gorp.stat(31), gorp.stat(32)
    assert 0 < fits <= limit, (fits, limit)
    return fits, limit


def sweep(batch, kernel, formats=(0, 1, 2), shifts=range(16), per_length=None, what=""):
    """The batch at every alignment in `shifts`, in every format: without a promise; with the promise of its longest line,
    synchronous and no_sync; and (per_length: ascending batches only) for every L of per_length the lines no longer than L under the
    promise L (the host takes the promise for L <= fits and a line of L units is left from fits + 1 to fits + 16 units on, by its
    skew: the small variants sweep L across all of that, the large ones, whose launches are long, the L a host off by one or two
    bytes would get wrong).  All these promises hold: gx_stat(h, 24) must not move -- a host that takes a promise the device then finds broken
    would count here.  The kernel that ran is the one named."""
    gorp = batch.gorp
    broken = gorp.stat(24)
    longest = int(batch.lens.max())
    for s in shifts:
        batch.place(s)
        for fmt in formats:
            batch.check(batch.launch(fmt), what + " no promise")
            assert gorp.stat(25) == kernel, (what, gorp.stat(25))
            batch.check(batch.launch(fmt, promise=longest), what + " promise %d (holds)" % longest)
            batch.check(batch.launch(fmt, promise=longest, no_sync=True), what + " promise %d (holds), no_sync" % longest)
            for L in per_length or ():
                n = int(np.searchsorted(batch.lens, L, side="right"))     # (ascending lengths: a prefix)
                assert n > 0 and batch.lens[n - 1] <= L and (n == batch.n or batch.lens[n] > L)
                batch.check(batch.launch(fmt, n=n, promise=L), what + " lines <= %d under promise %d (holds)" % (L, L))
            assert gorp.stat(25) == kernel
            assert gorp.stat(24) == broken, "%s, format %d, alignment %d: a promise that holds was counted as broken (host and device disagree " \
                                            "about the line that fits)" % (what, fmt, s)


def with_short_lines(lines, short, seed):
    """Every line followed by one to three short ones: the lane ranges of the tile kernel's rounds vary."""
    rng = random.Random(seed)
    out = []
    for ln in lines:
        out.append(ln)
        out.extend([short] * rng.randrange(1, 4))
    return out


def readme_batch(gorp, orc, lines, **kw):
    """README-definition lines (str, or bytes that keep their terminators with strip_eol) and the oracle's answers, which must show
    what the sweeps rely on: every HEAD line matches extraction 1 and its last capture ends at the line's end."""
    data, offsets = lines_to_csr(lines)
    if kw.get("strip_eol"):
        want_off, bodies, _ = O.read_lines(data)
        assert len(bodies) == len(lines), "read_lines returns as many lines as were joined"
        assert np.array_equal(want_off, offsets.astype(np.uint64))
        cd, co = lines_to_csr(bodies)
    else:
        bodies, (cd, co) = lines, (data, offsets)
    omid, ocaps = orc.extract_batch(cd, co, nthreads=16)
    body_len = np.diff(co.astype(np.int64))
    heads = np.array([(b if isinstance(b, str) else b.decode("latin-1")).startswith(HEAD) for b in bodies])
    assert heads.any() and (omid[heads] == 1).all() and (ocaps[heads, 7] == body_len[heads]).all()
    return DeviceBatch(gorp, data, offsets, omid, ocaps, **kw)


# ---- a. the staging edge, every length, every alignment ----------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, N.GX_CREATE_TIER_L2], ids=["lds", "l2"])
def test_staging_edge_every_length_every_alignment(flags):
    """Tile kernel, 4 KB staging area (line_bytes_hint = 20): every length from 15 to 4 200 bytes, ascending (64 near-edge lines share
    a group: many rounds, the last ones alone) and mixed with short lines, at all 16 byte alignments, in all three formats; and for
    every L across the host's edge the lines <= L under the promise L.  flags: dense rows in LDS, and rows in global memory."""
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition, flags=flags), oracle_for(definition)
    lo, hi = 15, 4200
    lines = [readme_line(k) for k in range(lo, hi + 1)]
    asc = readme_batch(gorp, orc, lines, kernel=N.GX_KERNEL_TILES, hint=20)
    assert int((asc.ocaps > 254).sum()) == sum(1 for k in range(lo, hi + 1) if k > 254)   # (one offset above 254 per line longer than that)
    fits, limit = edge_of(gorp, asc, N.GX_KERNEL_TILES)
    assert lo < fits and limit < hi, "the sweep does not bracket the edge: fits %d, limit %d" % (fits, limit)
    assert limit <= 4096
    sweep(asc, N.GX_KERNEL_TILES, per_length=range(fits - 8, limit - 48 + 9), what="ascending")
    mixed = readme_batch(gorp, orc, with_short_lines(lines, SHORT, 5), kernel=N.GX_KERNEL_TILES, hint=20)
    sweep(mixed, N.GX_KERNEL_TILES, what="with short lines")


def test_staging_edge_with_terminators():
    """strip_eol: the terminator is staged with the line, so the edge moves by its length.  Every body length 15..4 200 with each of
    "\\n", "\\r\\n" and "\\r" behind it; the promise speaks of the line with its terminator."""
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition), oracle_for(definition)
    lo, hi = 15, 4200
    lines = [(readme_line(k) + e).encode("latin-1") for k in range(lo, hi + 1) for e in ENDS]
    lines.sort(key=len)                                   # (ascending in memory: per_length takes prefixes)
    asc = readme_batch(gorp, orc, lines, kernel=N.GX_KERNEL_TILES, hint=20, strip_eol=True)
    fits, limit = edge_of(gorp, asc, N.GX_KERNEL_TILES)
    assert lo + 2 < fits and limit < hi
    sweep(asc, N.GX_KERNEL_TILES, per_length=range(fits - 8, limit - 48 + 9), what="terminated, ascending")
    mixed = with_short_lines(lines, (SHORT + "\r\n").encode("latin-1"), 6)
    sweep(readme_batch(gorp, orc, mixed, kernel=N.GX_KERNEL_TILES, hint=20, strip_eol=True), N.GX_KERNEL_TILES,
          what="terminated, with short lines")


def test_staging_edge_of_the_hop_tile_kernel():
    """GX_KERNEL_HOPS on the 64-extraction syslog definition: lengths 160..4 200 with a stride, every length within 80 of the edge."""
    rules, meta = W.syslog_definition(64, seed=3)
    gorp, orc = Gorp.construct(rules), oracle_for(rules)
    assert gorp.stat(14) > 0
    lo, hi = 160, 4200

    def batch(lengths, short_lines=False):
        parts = []
        rng = random.Random(4)
        for k in lengths:
            parts.append(W.syslog_lines(meta, 1, seed=70 + k % 97, line_bytes=k, corrupt_frac=0.0)[:2])
            if short_lines:
                parts.append(W.syslog_lines(meta, rng.randrange(1, 4), seed=k, line_bytes=160, corrupt_frac=0.0)[:2])
        data, offsets = join_csr(parts)
        lens = np.diff(offsets.astype(np.int64))
        if not short_lines:
            assert lens.tolist() == list(lengths), "the generator honours line_bytes"
        omid, ocaps = orc.extract_batch(data, offsets, nthreads=16)
        assert (omid >= 0).all() and (ocaps.max(axis=1) == lens).all()    # every line matches; its largest offset is its length
        return DeviceBatch(gorp, data, offsets, omid, ocaps, kernel=N.GX_KERNEL_HOPS, hint=20)

    fits, limit = edge_of(gorp, batch(range(lo, hi + 1, 101)), N.GX_KERNEL_HOPS)
    assert lo < fits - 80 and limit + 80 < hi, "the sweep does not bracket the edge: fits %d, limit %d" % (fits, limit)
    lengths = sorted(set(range(lo, hi + 1, 37)) | set(range(fits - 80, limit - 48 + 81)))
    sweep(batch(lengths), N.GX_KERNEL_HOPS, per_length=range(fits - 8, limit - 48 + 9), what="hop tile kernel, ascending")
    sweep(batch(lengths, short_lines=True), N.GX_KERNEL_HOPS, what="hop tile kernel, with short lines")


def utf16_csr(strings):
    units = [np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16) for s in strings]
    offsets = np.zeros(len(strings) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(u) for u in units])
    return np.concatenate(units), offsets


WIDE_UNIT = "\u4e2d"


def utf16_batch(gorp, orc, strings, **kw):
    """Strings as UTF-16 code units and the oracle on the Strings: a String of units <= 0xFF is its Latin-1 bytes (one batch); the
    ones that hold WIDE_UNIT one by one.  -> (batch, number of lines with a unit above 0xFF)."""
    data, offsets = utf16_csr(strings)
    omid, ocaps = orc.extract_batch(*lines_to_csr([s if WIDE_UNIT not in s else "" for s in strings]), nthreads=16)
    lens = np.diff(offsets.astype(np.int64))
    heads = np.array([s.startswith(HEAD) and WIDE_UNIT not in s for s in strings])
    assert (omid[heads] == 1).all() and (ocaps[heads, 7] == lens[heads]).all()
    n_wide = 0
    for i, s in enumerate(strings):
        if WIDE_UNIT in s:
            m, spans = orc.extract(s)
            omid[i], ocaps[i] = m, -1
            for g, span in enumerate(spans):
                if span is not None:
                    ocaps[i, 2 * g], ocaps[i, 2 * g + 1] = span
            n_wide += 1
    return DeviceBatch(gorp, data, offsets, omid, ocaps, utf16=True, **kw), n_wide


def with_wide_unit(s):
    return s[:len(s) // 2] + WIDE_UNIT + s[len(s) // 2 + 1:]


def test_staging_edge_utf16():
    """utf16: the tile kernel reads the code units itself and stages their low bytes; its staging area is 13 KB whatever the hint, and
    the skew counts units over a 32-byte chunk.  Lengths 15..13 400 units with a stride, every length within 80 of the edge, at unit
    alignments 0..15; every third near-edge line also holds a unit above 0xFF -- a line that is both left by the tile kernel and
    flagged for the per-line walk must be answered once, and so must one that is staged and flagged (exact overflow counts)."""
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition), oracle_for(definition)
    lo, hi = 15, 13400
    kw = dict(kernel=N.GX_KERNEL_TILES, hint=20)
    fits, limit = edge_of(gorp, utf16_batch(gorp, orc, [readme_line(k) for k in range(lo, hi + 1, 211)], **kw)[0], N.GX_KERNEL_TILES)
    assert lo < fits - 80 and limit + 80 < hi, "the sweep does not bracket the edge: fits %d, limit %d" % (fits, limit)
    lengths = sorted(set(range(lo, hi + 1, 211)) | set(range(fits - 80, limit - 48 + 81)))
    strings = [with_wide_unit(readme_line(k)) if k >= fits - 80 and k % 3 == 0 else readme_line(k) for k in lengths]
    asc, n_wide = utf16_batch(gorp, orc, strings, **kw)
    assert n_wide >= 50
    sweep(asc, N.GX_KERNEL_TILES, per_length=range(fits - 2, fits + 4), what="utf16, ascending")
    sweep(utf16_batch(gorp, orc, with_short_lines(strings, SHORT, 8), **kw)[0], N.GX_KERNEL_TILES, what="utf16, with short lines")


@pytest.mark.parametrize("flags,kernel", [(0, N.GX_KERNEL_TILES), (N.GX_CREATE_TIER_HOP, N.GX_KERNEL_HOPS), (N.GX_CREATE_TIER_HOP, N.GX_KERNEL_HOP_SLICES)],
                         ids=["tiles", "hops", "hop_slices"])
def test_utf16_lines_with_wide_units_are_counted_once(flags, kernel):
    """The kernels that read UTF-16 code units themselves walk a line's low bytes and flag the line when it holds a unit above 0xFF:
    the per-line walk then answers it.  Its clipped offsets are counted by that walk alone (found by the sweep above: the batch
    kernel's row from the low bytes counted them a first time).  Lines of 200..700 units, every second one with such a unit, u8 rows."""
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition, flags=flags), oracle_for(definition)
    strings = [with_wide_unit(readme_line(k)) if k % 2 else readme_line(k) for k in range(200, 701)]
    batch, n_wide = utf16_batch(gorp, orc, strings, kernel=kernel, hint=200)
    assert n_wide == 250 and int((batch.ocaps > 254).sum()) >= len(strings) - 60
    for s in (0, 3):
        batch.place(s)
        for fmt in (2, 1, 0):
            batch.check(batch.launch(fmt), "utf16 lines with wide units")
            assert gorp.stat(25) == kernel


@pytest.mark.parametrize("hint,area", [(200, 13), (250, 16)])
def test_staging_edge_of_the_larger_variants(hint, area):
    """The 13 KB (line_bytes_hint = 200) and 16 KB (250) byte variants of the tile kernel: lengths 11 800..16 500 with a stride at four
    alignments, every length within 80 of the edge at all sixteen."""
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition), oracle_for(definition)
    lo, hi = 11800, 16500
    whole = readme_batch(gorp, orc, [readme_line(k) for k in range(lo, hi + 1, 7)], kernel=N.GX_KERNEL_TILES, hint=hint)
    fits, limit = edge_of(gorp, whole, N.GX_KERNEL_TILES)
    assert lo < fits - 80 and limit + 80 < hi, "the sweep does not bracket the edge: fits %d, limit %d" % (fits, limit)
    assert (area - 1) * 1024 < limit <= area * 1024, "line_bytes_hint %d: a staging area of %d bytes, not the %d KB variant" % (hint, limit, area)
    sweep(whole, N.GX_KERNEL_TILES, formats=(0, 2), shifts=(0, 5, 10, 15), what="%d KB variant, the whole range" % area)
    # near the edge: every length at all sixteen alignments in int32 rows, the compact formats at four (a round of these lines is one
    # line of 13-16 KB walked by one wave: the launches are long); the promises L that the host can get wrong by one or two bytes
    few = (0, 5, 10, 15)
    band = [readme_line(k) for k in range(fits - 80, limit - 48 + 81)]
    asc = readme_batch(gorp, orc, band, kernel=N.GX_KERNEL_TILES, hint=hint)
    sweep(asc, N.GX_KERNEL_TILES, formats=(0,), per_length=range(fits - 2, fits + 4), what="%d KB variant, near the edge" % area)
    sweep(asc, N.GX_KERNEL_TILES, formats=(1, 2), shifts=few, per_length=range(fits - 2, fits + 4), what="%d KB variant, near the edge" % area)
    mixed = readme_batch(gorp, orc, with_short_lines(band, SHORT, 7), kernel=N.GX_KERNEL_TILES, hint=hint)
    sweep(mixed, N.GX_KERNEL_TILES, formats=(0,), what="%d KB variant, near the edge, with short lines" % area)
    sweep(mixed, N.GX_KERNEL_TILES, formats=(1, 2), shifts=few, what="%d KB variant, near the edge, with short lines" % area)


# ---- b. the 16-bit edge with terminators -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [N.GX_KERNEL_LANES, N.GX_KERNEL_HOP_SLICES], ids=["lanes", "hop_slices"])
def test_16_bit_edge_with_terminators(kernel):
    """The lane and hop slice kernels leave a line longer than their 16-bit positions -- judged WITHOUT its terminator, while a
    promise speaks of the line with it.  Bodies of 65 533..65 537 bytes ended by "\\n", "\\r\\n", "\\r" and nothing: a body of 65 535
    bytes + "\\r\\n" is 65 537 bytes in memory and is the batch kernel's to answer, once.  int32 and u16 rows (offset 65 535 does
    not fit a u16 row: stored as 65 534 and counted); no promise, and the lines <= L under the promise L for every L around the edge."""
    bodies = range(65533, 65538)
    if kernel == N.GX_KERNEL_LANES:
        definition = W.readme3_definition()
        gorp = Gorp.construct(definition, flags=N.GX_CREATE_TIER_RECORDS)
        body = {k: readme_line(k).encode("latin-1") for k in bodies}
        filler = [SHORT.encode("latin-1") + b"\n"] * 70
    else:
        definition, meta = W.syslog_definition(64, seed=3)
        gorp = Gorp.construct(definition)
        assert gorp.stat(19) > 0
        body = {}
        for k in bodies:
            d, o, _ = W.syslog_lines(meta, 1, seed=70 + k % 97, line_bytes=k, corrupt_frac=0.0)
            body[k] = bytes(d[o[0]:o[1]])
            assert len(body[k]) == k
        d, o, _ = W.syslog_lines(meta, 70, seed=7, line_bytes=160, corrupt_frac=0.0)
        filler = [bytes(d[o[i]:o[i + 1]]) + b"\n" for i in range(70)]
    orc = oracle_for(definition)
    lines = sorted([body[k] + e.encode("latin-1") for k in bodies for e in ENDS + ("",)], key=len)
    n_long = len(lines)
    # ascending long lines first (per-L prefixes), the short ones behind and in front of every prefix through `first`
    raw = filler + lines + filler
    data, offsets = lines_to_csr(raw)
    stripped = [ln.rstrip(b"\r\n") for ln in raw]
    assert all(len(s) >= len(r) - 2 and not s.endswith((b"\r", b"\n")) for s, r in zip(stripped, raw))
    omid, ocaps = orc.extract_batch(*lines_to_csr(stripped), nthreads=16)
    long_rows = slice(len(filler), len(filler) + n_long)
    assert (omid >= 0).all() and ocaps[long_rows].max(axis=1).tolist() == [len(s) for s in stripped[long_rows]]
    if kernel == N.GX_KERNEL_LANES:   # (README lines: extraction 1, the last capture ends at the line's end)
        assert (omid[long_rows] == 1).all() and ocaps[long_rows, 7].tolist() == [len(s) for s in stripped[long_rows]]
    batch = DeviceBatch(gorp, data, offsets, omid, ocaps, kernel=kernel, hint=200, strip_eol=True)
    broken = gorp.stat(24)
    for s in (0, 1, 7, 15):
        batch.place(s)
        for fmt in (0, 1):
            batch.check(batch.launch(fmt), "no promise")
            assert gorp.stat(25) == kernel
            assert gorp.stat(32) in (65534, 65535), gorp.stat(32)
            for L in range(65531, 65541):
                n = len(filler) + sum(1 for ln in lines if len(ln) <= L)
                batch.check(batch.launch(fmt, n=n, promise=L), "lines <= %d under promise %d" % (L, L))
                batch.check(batch.launch(fmt, n=n, promise=L, no_sync=True), "lines <= %d under promise %d, no_sync" % (L, L))
            assert gorp.stat(24) == broken, "a promise that holds was counted as broken"


# ---- c. broken promises, every format, every entry ---------------------------------------------------------------------------

LONG_AT = 1234


def promise_lines(big):
    rng = random.Random(77)
    lines = ["[123456789]: %s 5ms /%s" % (rng.choice(["GET", "PUT", "HEAD"]), "x" * rng.randrange(1, 150)) for _ in range(5000)]
    lines[LONG_AT] = "[123456789]: GET 5ms /" + "y" * big
    return lines


def assert_left_unwritten(batch, launched, left, what):
    """A no_sync batch whose promise broke: the rows of `left` still hold the sentinel, every other row is the oracle's, and the
    overflow counter has the other lines' offsets only."""
    batch.torch.cuda.synchronize()
    fmt, n = launched[0], launched[1]
    gm, gc, gover = batch.read(launched)
    wm, wc, _ = batch.want(fmt, n)
    rest = np.ones(n, bool)
    rest[left] = False
    assert np.array_equal(gm[rest], wm[rest]) and np.array_equal(gc[rest], wc[rest]), what + ": a row beside the long line's differs from the oracle"
    fill = -7 if fmt == 0 else 7
    assert (gm[left] == fill).all() and (gc[left] == fill).all(), what + ": the long line's row was written (%s %s)" % (gm[left], gc[left])
    if fmt:
        want = int((batch.ocaps[:n][rest] > ROW_LIMIT[fmt]).sum())
        assert gover == want, "%s: overflow counter %d, the other lines have %d offsets above %d" % (what, gover, want, ROW_LIMIT[fmt])


_PROMISE_KERNELS = [(0, 0), (N.GX_CREATE_TIER_L2, 0), (N.GX_CREATE_TIER_RECORDS, N.GX_KERNEL_LANES), (N.GX_CREATE_TIER_HOP, 0),
                    (N.GX_CREATE_TIER_HOP, N.GX_KERNEL_HOP_SLICES)]


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("flags,kernel", _PROMISE_KERNELS)
def test_broken_promise_compact_rows(flags, kernel, fmt):
    """What test_max_line_bytes_promise checks for int32 rows, for u16 and u8 rows with their overflow counter: a synchronous call
    makes good (rows and counter exact, gx_stat(h, 24) + 1); a no_sync call leaves the long line's row unwritten and uncounted, and
    the next call on the stream raises."""
    import torch
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition, flags=flags), oracle_for(definition)
    lines = promise_lines(70000 if kernel in (N.GX_KERNEL_LANES, N.GX_KERNEL_HOP_SLICES) else 20000)
    data, offsets = lines_to_csr(lines)
    omid, ocaps = orc.extract_batch(data, offsets, nthreads=8)
    assert omid[LONG_AT] == 1 and ocaps[LONG_AT, 7] == len(lines[LONG_AT])
    if len(lines[LONG_AT]) > ROW_LIMIT[fmt]:     # (u8 rows always; u16 rows under the kernels whose long line is 70 000 bytes)
        assert int((ocaps[LONG_AT] > ROW_LIMIT[fmt]).sum()) >= 1
    batch = DeviceBatch(gorp, data, offsets, omid, ocaps, kernel=kernel, hint=200)
    st = torch.cuda.current_stream().cuda_stream
    batch.check(batch.launch(fmt, stream=st), "no promise")
    batch.check(batch.launch(fmt, promise=len(lines[LONG_AT]), stream=st), "a promise that holds")
    assert gorp.stat(24) == 0
    batch.check(batch.launch(fmt, promise=200, stream=st), "synchronous call, broken promise (made good)")
    assert gorp.stat(24) == 1
    assert_left_unwritten(batch, batch.launch(fmt, promise=200, no_sync=True, stream=st), [LONG_AT], "no_sync call, broken promise")
    with pytest.raises(G.GorpError, match="max_line_bytes"):
        batch.launch(fmt, stream=st)
    assert gorp.stat(24) == 2
    batch.check(batch.launch(fmt, stream=st), "after the report")
    assert gorp.stat(24) == 2


@pytest.mark.parametrize("fmt", [1, 2])
def test_broken_promise_multi_device_counts_every_line_once(fmt):
    """gx_extract_batch_multi_device waits for its shards itself: a shard whose promise broke is made good before the call returns
    -- its rows AND its overflow counter.  Three handles on device 0, the long line in the first shard, a counter per shard."""
    import torch
    definition = W.readme3_definition()
    gorps, orc = [Gorp.construct(definition) for _ in range(3)], oracle_for(definition)
    lines = promise_lines(20000)
    data, offsets = lines_to_csr(lines)
    omid, ocaps = orc.extract_batch(data, offsets, nthreads=8)
    d, o = torch.from_numpy(data).cuda(), torch.from_numpy(offsets).cuda()
    cuts = [0, 1700, 3400, 5000]
    outs, shards = [], []
    for k, g in enumerate(gorps):
        a, n = cuts[k], cuts[k + 1] - cuts[k]
        rows = torch.full((n, 9), 7, dtype=torch.int16 if fmt == 1 else torch.uint8, device="cuda")
        over = torch.zeros(1, dtype=torch.int64, device="cuda")
        outs.append((rows, over))
        shards.append((g, d.data_ptr(), o.data_ptr() + 4 * a, n, None, rows.data_ptr(), over.data_ptr(), None))
    torch.cuda.synchronize()
    G.extract_batch_multi_device(shards, compact=fmt, line_bytes_hint=200, max_line_bytes=200)
    torch.cuda.synchronize()
    assert [g.stat(24) for g in gorps] == [1, 0, 0]
    for k, (rows, over) in enumerate(outs):
        a, b = cuts[k], cuts[k + 1]
        m, c = G.unpack_rows(rows.cpu().numpy().view(np.uint16 if fmt == 1 else np.uint8))
        big = ocaps[a:b] > ROW_LIMIT[fmt]
        assert np.array_equal(m, omid[a:b]) and np.array_equal(c, np.where(big, ROW_LIMIT[fmt], ocaps[a:b])), "shard %d: rows differ from the oracle" % k
        assert int(over.item()) == int(big.sum()), "shard %d (%s): overflow counter %d after the make-good, the oracle has %d offsets above %d" % (
            k, "holds the long line" if a <= LONG_AT < b else "all lines short", int(over.item()), int(big.sum()), ROW_LIMIT[fmt])


@pytest.mark.parametrize("flags", [0, N.GX_CREATE_TIER_HOP], ids=["lds", "hop"])
def test_broken_promise_utf16(flags):
    """utf16 on the two layouts that read the code units without a copy: the promise counts units; broken, it is made good or
    reported as for bytes."""
    import torch
    definition = W.readme3_definition()
    gorp, orc = Gorp.construct(definition, flags=flags), oracle_for(definition)
    lines = promise_lines(20000)
    omid, ocaps = orc.extract_batch(*lines_to_csr(lines), nthreads=8)
    data, offsets = utf16_csr(lines)
    batch = DeviceBatch(gorp, data, offsets, omid, ocaps, hint=200, utf16=True)
    st = torch.cuda.current_stream().cuda_stream
    for fmt in (0, 2):
        before = gorp.stat(24)
        batch.check(batch.launch(fmt, promise=len(lines[LONG_AT]), stream=st), "utf16, a promise that holds")
        assert gorp.stat(25) in (N.GX_KERNEL_TILES, N.GX_KERNEL_HOPS) and gorp.stat(24) == before
        batch.check(batch.launch(fmt, promise=200, stream=st), "utf16, synchronous call, broken promise (made good)")
        assert gorp.stat(24) == before + 1
        assert_left_unwritten(batch, batch.launch(fmt, promise=200, no_sync=True, stream=st), [LONG_AT], "utf16, no_sync call, broken promise")
        with pytest.raises(G.GorpError, match="max_line_bytes"):
            batch.launch(fmt, stream=st)
        assert gorp.stat(24) == before + 2
        batch.check(batch.launch(fmt, stream=st), "utf16, after the report")


# ---- d. stacked batches ------------------------------------------------------------------------------------------------------

class Stack:
    """Two batches of README lines on one handle -- `breaks` holds one line of 20 000 bytes (a promise of 200 is broken), `holds`
    none -- and streams that can be held busy, so that batches queue behind one another before the host looks."""

    def __init__(self, n_handles=1):
        import torch
        self.torch = torch
        definition = W.readme3_definition()
        self.gorps, orc = [Gorp.construct(definition) for _ in range(n_handles)], oracle_for(definition)
        self.gorp = self.gorps[0]
        lines = promise_lines(20000)
        short = [ln for i, ln in enumerate(lines) if i != LONG_AT]
        self.breaks = DeviceBatch(self.gorp, *lines_to_csr(lines), *orc.extract_batch(*lines_to_csr(lines), nthreads=8), hint=200)
        self.holds = DeviceBatch(self.gorp, *lines_to_csr(short), *orc.extract_batch(*lines_to_csr(short), nthreads=8), hint=200)
        self.ballast = torch.ones(64 << 20, dtype=torch.float32, device="cuda")
        # how many passes over the ballast keep a stream busy for about 300 ms (bounded: at most 4000 small kernels)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            self.ballast.mul_(1.0)
        t1.record()
        torch.cuda.synchronize()
        self.passes = int(min(4000, max(40, 300.0 / max(t0.elapsed_time(t1) / 20, 1e-3))))

    def hold(self, stream):
        with self.torch.cuda.stream(stream):
            for _ in range(self.passes):
                self.ballast.mul_(1.0)

    def still_queued(self, stream):
        """An event behind everything enqueued so far: un-signalled now means the batches before it have not run."""
        ev = self.torch.cuda.Event()
        ev.record(stream)
        return ev

    def call(self, batch, fmt=0, **kw):
        """One call into buffers that outlive it; -> (the buffers, the GorpError or None).  Any other error is the test's."""
        out = batch.buffers(fmt)
        try:
            batch.launch(fmt, into=out, **kw)
            return out, None
        except G.GorpError as e:
            assert "max_line_bytes" in str(e), e
            return out, e


def check_own_rows(batch, out, err, what):
    """What a synchronous call owes whether or not it reports an earlier batch: returned without error, or with the error of the call
    that waited for its own batch ("this batch itself is complete") -- every row and the overflow counter are the oracle's, a broken
    promise of its own made good; refused at submission ("was not launched") -- nothing written."""
    if err is not None and "was not launched" in str(err):
        batch.check_not_launched(out, what)
        return False
    assert err is None or "itself is complete" in str(err), err
    batch.check(out, what + (": raised for an earlier batch, its own rows" if err is not None else ": returned without error"))
    return True


def clean_calls_stay_clean(stack, stream, what):
    for q in range(2):
        out, err = stack.call(stack.holds, stream=stream.cuda_stream)
        assert err is None, "%s: clean call %d after the report raised again: %s" % (what, q + 1, err)
        stack.holds.check(out, what + ": clean call")


def test_stacked_no_sync_break_then_synchronous_break():
    """A (no_sync) breaks its promise and is still queued when B (synchronous, same stream) is submitted; B breaks its own too.  B's
    rows are complete when it returns, and A's unwritten row is reported by B or by the next call."""
    stack = Stack()
    torch, gorp = stack.torch, stack.gorp
    s = torch.cuda.Stream()
    before = gorp.stat(24)
    stack.hold(s)
    a, err = stack.call(stack.breaks, promise=200, no_sync=True, stream=s.cuda_stream)
    assert err is None
    ev = stack.still_queued(s)
    assert not ev.query(), "batch A had run before B was submitted: the interleaving was missed"
    out_b, err_b = stack.call(stack.breaks, fmt=2, promise=200, stream=s.cuda_stream)
    s.synchronize()
    assert_left_unwritten(stack.breaks, a, [LONG_AT], "batch A (no_sync, broken promise)")
    assert check_own_rows(stack.breaks, out_b, err_b, "batch B (synchronous, u8 rows, broken promise)"), "A was still queued: B was launched"
    if err_b is None:
        out_c, err_c = stack.call(stack.holds, stream=s.cuda_stream)
        assert err_c is not None, "batch A (no_sync) left a row unwritten and nobody reported it: B returned without error and so did the " \
                                  "first call after the stream had drained"
    assert gorp.stat(24) >= before + 2, "two batches broke their promise (one error, one make-good): gx_stat(h, 24) went from %d to %d" % (before, gorp.stat(24))
    clean_calls_stay_clean(stack, s, "A no_sync breaks, B synchronous breaks")


def test_stacked_no_sync_break_then_synchronous_hold():
    """A (no_sync) breaks and is still queued when B (synchronous, promise holds) is submitted: B or the next call reports A."""
    stack = Stack()
    torch, gorp = stack.torch, stack.gorp
    s = torch.cuda.Stream()
    before = gorp.stat(24)
    stack.hold(s)
    a, err = stack.call(stack.breaks, promise=200, no_sync=True, stream=s.cuda_stream)
    assert err is None
    ev = stack.still_queued(s)
    assert not ev.query(), "batch A had run before B was submitted: the interleaving was missed"
    out_b, err_b = stack.call(stack.holds, fmt=1, promise=200, stream=s.cuda_stream)
    s.synchronize()
    assert_left_unwritten(stack.breaks, a, [LONG_AT], "batch A (no_sync, broken promise)")
    assert check_own_rows(stack.holds, out_b, err_b, "batch B (synchronous, u16 rows, promise holds)"), "A was still queued: B was launched"
    if err_b is None:
        out_c, err_c = stack.call(stack.holds, stream=s.cuda_stream)
        assert err_c is not None, "batch A (no_sync) left a row unwritten and nobody reported it: B returned without error and so did the " \
                                  "first call after the stream had drained"
    assert gorp.stat(24) == before + 1, "one batch broke its promise: gx_stat(h, 24) went from %d to %d" % (before, gorp.stat(24))
    clean_calls_stay_clean(stack, s, "A no_sync breaks, B synchronous holds")
    assert gorp.stat(24) == before + 1


def test_stacked_two_no_sync_breaks_then_a_call_without_promise():
    """A and B (both no_sync) break and are still queued when C (synchronous, no promise) is submitted: C (or B) raises; after it a
    clean call succeeds and a further one does not raise again."""
    stack = Stack()
    torch, gorp = stack.torch, stack.gorp
    s = torch.cuda.Stream()
    before = gorp.stat(24)
    stack.hold(s)
    a, err_a = stack.call(stack.breaks, promise=200, no_sync=True, stream=s.cuda_stream)
    b, err_b = stack.call(stack.breaks, fmt=2, promise=200, no_sync=True, stream=s.cuda_stream)
    assert err_a is None
    ev = stack.still_queued(s)
    assert not ev.query(), "batches A and B had run before C was submitted: the interleaving was missed"
    c, err_c = stack.call(stack.breaks, stream=s.cuda_stream)
    s.synchronize()
    assert_left_unwritten(stack.breaks, a, [LONG_AT], "batch A (no_sync, broken promise)")
    assert err_b is None, "A was still queued: B was launched"
    assert_left_unwritten(stack.breaks, b, [LONG_AT], "batch B (no_sync, u8 rows, broken promise)")
    assert check_own_rows(stack.breaks, c, err_c, "batch C (synchronous, no promise)"), "A and B were still queued: C was launched"
    assert err_b is not None or err_c is not None, "batches A and B (no_sync) left rows unwritten and neither B nor C reported it"
    assert gorp.stat(24) >= before + 1
    clean_calls_stay_clean(stack, s, "A and B no_sync break, C synchronous without a promise")


@pytest.mark.parametrize("b_breaks", [False, True], ids=["b_holds", "b_breaks"])
def test_stacked_multi_device_break_then_multi_device_call(b_breaks):
    """A = gx_extract_batch_multi_device(no_sync) on the caller's stream breaks and is still queued when B = the same entry,
    synchronous, is submitted -- with a promise that holds (B's shard needs no second run) or one that B breaks itself (made good:
    u8 rows and the shard's counter exact).  A's unwritten row is reported by B or by the next call on the stream."""
    stack = Stack()
    torch, gorp = stack.torch, stack.gorp
    s = torch.cuda.Stream()
    before = gorp.stat(24)

    def shard(batch, fmt):
        out = batch.buffers(fmt)
        _, n, mid, rows, over = out
        return out, [(gorp, batch.ptr, batch.o.data_ptr(), n, mid.data_ptr() if fmt == 0 else None, rows.data_ptr(),
                      over.data_ptr() if fmt else None, s.cuda_stream)]

    batch_b = stack.breaks if b_breaks else stack.holds
    out_a, shards_a = shard(stack.breaks, 0)
    out_b, shards_b = shard(batch_b, 2)
    torch.cuda.synchronize()
    stack.hold(s)
    G.extract_batch_multi_device(shards_a, line_bytes_hint=200, max_line_bytes=200, no_sync=True)
    ev = stack.still_queued(s)
    assert not ev.query(), "batch A had run before B was submitted: the interleaving was missed"
    err_b = None
    try:
        G.extract_batch_multi_device(shards_b, compact=2, line_bytes_hint=200, max_line_bytes=200)
    except G.GorpError as e:
        assert "max_line_bytes" in str(e), e
        err_b = e
    s.synchronize()
    assert_left_unwritten(stack.breaks, out_a, [LONG_AT], "batch A (multi-device entry, no_sync, broken promise)")
    assert check_own_rows(batch_b, out_b, err_b, "batch B (multi-device entry, synchronous, u8 rows, promise %s)" % ("broken" if b_breaks else "holds")), \
        "A was still queued: B was launched"
    if err_b is None:
        out_c, err_c = stack.call(stack.holds, stream=s.cuda_stream)
        assert err_c is not None, "batch A (multi-device entry, no_sync) left a row unwritten and nobody reported it: B returned without " \
                                  "error and so did the first call after the stream had drained; gx_stat(h, 24) went from " \
                                  "%d to %d" % (before, gorp.stat(24))
    want = before + 1 + (1 if b_breaks else 0)
    assert gorp.stat(24) == want, "%d batch(es) broke their promise: gx_stat(h, 24) went from %d to %d" % (want - before, before, gorp.stat(24))
    clean_calls_stay_clean(stack, s, "multi-device A no_sync breaks, multi-device B")


def test_two_streams_report_their_own_breaks():
    """Two streams of one handle, a broken no_sync promise on each: each stream's next call reports its own, neither the other's."""
    stack = Stack()
    torch, gorp = stack.torch, stack.gorp
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # (each stream has had a launch: it owns its slot)
    for s in (s1, s2):
        stack.holds.check(stack.call(stack.holds, stream=s.cuda_stream)[0], "first launch of a stream")
    before = gorp.stat(24)
    a, err = stack.call(stack.breaks, promise=200, no_sync=True, stream=s1.cuda_stream)
    assert err is None
    s1.synchronize()
    # stream 2 is not told of stream 1's break
    out, err = stack.call(stack.holds, promise=200, stream=s2.cuda_stream)
    assert err is None, "stream 2 was told of stream 1's break"
    stack.holds.check(out, "stream 2, clean")
    b, err = stack.call(stack.breaks, fmt=2, promise=200, no_sync=True, stream=s2.cuda_stream)
    assert err is None
    s2.synchronize()
    assert gorp.stat(24) == before
    for name, s, left in (("stream 1", s1, a), ("stream 2", s2, b)):
        assert_left_unwritten(stack.breaks, left, [LONG_AT], name + " (no_sync, broken promise)")
        out, err = stack.call(stack.holds, stream=s.cuda_stream)
        assert err is not None, name + ": the no_sync batch left a row unwritten and the stream's next call did not report it"
        clean_calls_stay_clean(stack, s, name)
    assert gorp.stat(24) == before + 2
