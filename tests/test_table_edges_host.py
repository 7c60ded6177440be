"""The table images of tests/table_edge_cases.py on host-only handles: which image every case has on either side of its format's
ceiling (so that a moved limit or a drift in the choice of tier shows without a GPU, and tests/test_gpu_table_edges.py cannot
quietly test other kernels), the product's tables against the oracle for the small cases, and that the lines of the dense-rows
cases do walk rows in the upper half of the LDS address space.  No kernel runs here."""
import numpy as np
import pytest

import table_edge_cases as TE
from blob_interp import Blob, units_of
from gorp_amd.gorp import Gorp, lines_to_csr
from oracle import oracle as O
from test_compiler_vs_oracle import extract_both_ways


def host(name, flags):
    return Gorp.construct(TE.definition(name)[0], host_only=True, flags=flags)


def oracle_for(rules):
    built = [e.build() for e in rules]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


def lines_of(batch):
    data, offsets = batch
    return [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)]


@pytest.mark.parametrize("name,flags", sorted(TE.EXPECT))
def test_every_case_has_the_image_it_is_meant_to_test(name, flags):
    """table_edge_cases.EXPECT, and per ceiling the arithmetic that puts the case where it is meant to be."""
    g = host(name, flags)
    TE.expected(g, name, flags)
    ncls, tier = g.stat(1), g.stat(7)
    row_bytes = (ncls + 3) * 4
    if name.startswith("classes"):
        assert ncls == len(TE.definition(name)[0])
        assert (tier in (3, 4)) == (ncls <= 250 and flags in (0, TE.REC, TE.RECG))       # range records: 250 classes at most
        assert (tier != 0) == (ncls <= 252)                                                # any image: 252
        assert g.stat(27) == (ncls if flags == TE.PROGRAMS else 0)
        assert (g.stat(35) > 0) == (flags == TE.PROGRAMS)        # (-1: no extraction runs as a program)
    if name.startswith("dense") and flags != TE.NO_FUSED:
        # the fused automaton's rows and the match automaton's in one image: successors are 16-bit LDS addresses
        rows = g.stat(38)
        assert g.stat(39) == 1
        assert (544 + rows * row_bytes <= 65536) == (tier == 1), (rows, row_bytes)
        if tier == 1:
            assert 544 + rows * row_bytes > 65536 - 5 * 1024 and 60 * 1024 < g.stat(12) <= 65536     # within 5 KB of the ceiling
    if name.startswith("dense") and flags == TE.NO_FUSED:
        assert g.stat(39) == 0 and tier == 1 and 544 + g.stat(38) * row_bytes <= 65536
    if name.startswith("records"):
        # 8 bytes a record: 80 extractions stay within the 96 KB of LDS, 96 do not
        assert (1088 + 8 * g.stat(36) <= 96 * 1024) == (tier == 3), g.stat(36)
        if tier == 3:
            assert 92 * 1024 < g.stat(12) <= 96 * 1024
    if name.startswith("wide") and flags in (TE.REC, TE.RECG):
        if name == "wide440":
            assert tier == 4 and 0xE000 < g.stat(36) <= 65535        # every successor still fits 16 bits
        if name == "wide_max":
            assert tier == 4 and g.stat(39) == 1 and 65535 < g.stat(36) < (1 << 22) and g.stat(37) <= 65535
            assert g.stat(38) <= 65536                               # (the fused automaton's states: 16 bits)
        if name == "wide_max+1":
            assert g.stat(36) == 0 and g.stat(39) == 0               # no fused automaton: no records, the two-pass layout
    if (name, flags) == ("wide_max", 0):
        assert g.stat(0) < 32768 and g.stat(39) == 1 and g.stat(14) == g.stat(38) - g.stat(0)
    if name in ("wide_max+1", "states570"):
        assert g.stat(39) == 0 and g.stat(38) == g.stat(0) + g.stat(2)          # one capture automaton per extraction
    if name == "states570":
        assert g.stat(0) == 33282 and g.stat(22) == (g.stat(0) if flags == 0 else 0)


SMALL = ["classes250", "classes251", "classes252", "classes253", "dense_1x13", "dense_1x14", "dense_2x6", "dense_2x7"]


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_agree_with_the_oracle(name):
    """The product's tables (tests/blob_interp.py walks the blob as the per-line kernel does: two passes, and the fused automaton)
    against the oracle on the case's own lines: all 3 000 of a class case, the first 600 of a dense-rows case."""
    rules, meta = TE.definition(name)
    b, orc = Blob(host(name, 0).blob()), oracle_for(rules)
    lines = TE.literal_lines(len(rules)) if meta is None else lines_of(TE.syslog_batch(meta, 600, seed=len(rules)))
    assert b.union_ok
    hits = 0
    for ln in lines:
        got, want = extract_both_ways(b, units_of(ln)), orc.extract(ln)
        assert got == want, (name, ln, got, want)
        hits += got[0] >= 0
    assert 10 * hits > len(lines)
    if meta is None:      # ... and with every extraction a program (GX_CREATE_PROGRAMS), which 253 classes leave as the only other way
        p = Blob(host(name, TE.PROGRAMS).blob())
        assert all(p.is_pike(k) for k in range(len(rules)))
        for ln in lines[::5]:
            assert p.extract(units_of(ln)) == orc.extract(ln), (name, ln)


@pytest.mark.parametrize("name", ["dense_1x13", "dense_2x6"])
def test_lines_walk_rows_in_the_upper_half_of_lds(name):
    """A successor is the LDS address of its row, 544 + row * (classes + 3) * 4, in a 16-bit field.  The match automaton's rows come
    first: its 113 / 114 states (Blob.match_state says where a line ends) all lie below 0x8000.  The fused automaton's rows follow
    -- state s is row m_states + s -- and it is those that capture batches walk: the lines of the case end in rows at and above
    0x8000, bit 15 of the field in use, and the deepest within a row or two of the image's last."""
    rules, meta = TE.definition(name)
    b = Blob(host(name, 0).blob())
    row_bytes = (b.ncls + 3) * 4
    rows = b.m_states + b.uni["n_states"]
    assert 544 + rows * row_bytes <= 65536 < 544 + (rows + 25) * row_bytes      # 25 rows from the ceiling
    assert 544 + b.m_states * row_bytes < 0x8000
    lines = lines_of(TE.syslog_batch(meta, 300, seed=len(rules)))
    match_ends = [b.match_state(units_of(ln)) for ln in lines]
    matched = [i for i, st in enumerate(match_ends) if b.m_accept_first[st] >= 0]
    assert len(matched) > 200 and all(st < b.m_states for st in match_ends)

    def fused_end(ln):      # (blob_interp: extract_union's walk, for the state it ends in)
        ts = 0
        for c in b.classes(units_of(ln)):
            ts = int(b.uni["trans"][ts, c]) & 0xFFFF
        return ts

    ends = [544 + (b.m_states + fused_end(lines[i])) * row_bytes for i in matched]
    assert all(a >= 0x8000 for a in ends), min(ends)
    assert max(ends) >= 544 + (rows - 3) * row_bytes, (max(ends), rows)
