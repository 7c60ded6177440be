"""Definitions and lines at the limits of the batch kernels' table images (gorp_amd/csrc/gx_images.cpp), for
tests/test_table_edges_host.py and tests/test_gpu_table_edges.py: not a conftest, nothing here runs a kernel.

Every image format has a ceiling that decides which kernel a definition gets, and a field that is full just below it:

    dense rows in LDS           544 + rows * (classes + 3) * 4 <= 65 536: a successor is the 16-bit LDS address of its row
    any image                   classes <= 252 (a column offset, class * 4 and three more columns, stays below 1 024)
    range records               classes <= 250 (class ids 254 and 255 are reserved)
    range records in LDS        96 KB, successors of 16 bits; in global memory successors of 22 bits
    the fused automaton         16-bit states; beyond it capture batches take the two-pass layout on rows in global memory
    match automaton             its states pass 2^15 at about 560 extractions of the syslog family

A case is a definition and the create flags it is built with; EXPECT says what gx_stat must report for it, so that a moved limit
or a drift in the choice of tier shows on the CPU (test_table_edges_host.py) and the GPU tests cannot quietly test other kernels.
The cases come in pairs, one on each side of a ceiling.

Lines are bytes (one Latin-1 code unit each)."""
import random

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction

L2, REC, RECG = N.GX_CREATE_TIER_L2, N.GX_CREATE_TIER_RECORDS, N.GX_CREATE_TIER_RECORDS_GLOBAL
PROGRAMS, NO_FUSED, RESIDENT = N.GX_CREATE_PROGRAMS, N.GX_CREATE_NO_FUSED, N.GX_CREATE_RESIDENT_ONE

# The largest syslog definition (seed 3) that still has the fused automaton (59 955 states) and with it range records in global
# memory under REC / RECG: 68 218 records.  With one extraction more no fused automaton is built.  Found by a host-only search;
# test_table_edges_host.py asserts both sides.
WIDE_MAX = 513


# ---- character classes -------------------------------------------------------------------------------------------------------
def literal_bytes(n):
    """The first n byte values of 1..255 without LF and CR (253 of them at most)."""
    return [b for b in range(1, 256) if b not in (10, 13)][:n]


def literal_definition(n):
    """n extractions "<byte>=" \\d+ over distinct bytes: every literal byte is a character class of its own ('=' and the digits are
    literals themselves from n = 61 on) -- n classes for the n used here (gx_stat 1, in EXPECT)."""
    return [FlattenedExtraction("r%d" % i, [["text", chr(b) + "="], ["extractor", "v", [["pattern", "\\d+"]]]]) for i, b in enumerate(literal_bytes(n))]


def literal_lines(n, n_lines=3000):
    """Every literal byte of literal_definition(n) in turn -- and the bytes that are no literal: NUL, LF, CR, 0xFF below 253 literals --
    followed by '=', '==' or nothing and 0-12 characters of 0123456789x; the last line is empty."""
    rng = random.Random(n)
    literals = literal_bytes(n)
    heads = literals + [b for b in (0x00, 0x0A, 0x0D, 0xFF) if b not in literals]
    lines = []
    for i in range(n_lines - 1):
        tail = "".join(rng.choice("0123456789x") for _ in range(rng.randint(0, 12)))
        lines.append(bytes([heads[i % len(heads)]]) + rng.choice([b"=", b"==", b""]) + tail.encode("latin-1"))
    return lines + [b""]


# ---- the syslog family -------------------------------------------------------------------------------------------------------
def syslog(n_rules, n_keys=7):
    """(rules, meta) of gorp_amd.workloads.syslog_definition at seed 3."""
    return W.syslog_definition(n_rules, seed=3, n_keys=n_keys)


def syslog_batch(meta, n_lines, seed, line_bytes=200, lengths=None):
    """(data, offsets) of W.syslog_lines with one line in ten damaged; lengths=(lo, hi): log-uniform line lengths instead of line_bytes."""
    kw = {} if lengths is None else {"min_len": lengths[0], "max_len": lengths[1]}
    data, offsets, _ = W.syslog_lines(meta, n_lines, seed=seed, line_bytes=line_bytes, corrupt_frac=0.1, **kw)
    return data, offsets


# name -> (what builds it, its arguments)
CASES = {
    "classes250": (literal_definition, (250,)), "classes251": (literal_definition, (251,)),
    "classes252": (literal_definition, (252,)), "classes253": (literal_definition, (253,)),
    "dense_1x13": (syslog, (1, 13)), "dense_1x14": (syslog, (1, 14)),      # one extraction of 13 / 14 keys
    "dense_2x6": (syslog, (2, 6)), "dense_2x7": (syslog, (2, 7)),
    "records80": (syslog, (80,)), "records96": (syslog, (96,)),
    "wide440": (syslog, (440,)), "wide_max": (syslog, (WIDE_MAX,)), "wide_max+1": (syslog, (WIDE_MAX + 1,)),
    "states570": (syslog, (570,)),
}


def definition(name):
    """(rules, meta): meta is what W.syslog_lines wants, None for the literal-byte definitions."""
    make, args = CASES[name]
    made = make(*args)
    return made if make is syslog else (made, None)


# (case, create flags) -> (gx_stat 1: character classes; 7: the tier of capture batches; 9: of match-only batches; whether 14 > 0:
# hop tables for capture batches; whether 22 > 0: for match-only batches; 26: why capture batches have none).
# Tiers: 1 dense rows in LDS, 2 dense rows in global memory, 3 range records in LDS, 4 range records in global memory, 0 no image.
EXPECT = {
    # 250 classes: the last definition with range records; 251, 252: dense rows in global memory whatever the flag; 253: no image
    ("classes250", 0): (250, 3, 3, True, True, 0), ("classes250", L2): (250, 2, 2, False, False, 4),
    ("classes250", REC): (250, 3, 3, False, False, 4), ("classes250", RECG): (250, 4, 4, False, False, 4),
    ("classes251", 0): (251, 2, 2, True, True, 0), ("classes251", L2): (251, 2, 2, False, False, 4),
    ("classes251", REC): (251, 2, 2, False, False, 4), ("classes251", RECG): (251, 2, 2, False, False, 4),
    ("classes252", 0): (252, 2, 2, True, True, 0), ("classes252", L2): (252, 2, 2, False, False, 4),
    ("classes252", REC): (252, 2, 2, False, False, 4), ("classes252", RECG): (252, 2, 2, False, False, 4),
    ("classes253", 0): (253, 0, 0, False, False, 4), ("classes253", L2): (253, 0, 0, False, False, 4),
    ("classes253", REC): (253, 0, 0, False, False, 4), ("classes253", RECG): (253, 0, 0, False, False, 4),
    ("classes253", PROGRAMS): (253, 0, 0, False, False, 4),
    # dense rows in LDS: 62 448 and 61 584 bytes of image; one key more and the rows leave LDS
    ("dense_1x13", 0): (43, 1, 1, False, False, 4), ("dense_1x14", 0): (44, 3, 3, True, True, 0),
    ("dense_2x6", 0): (42, 1, 1, False, False, 4), ("dense_2x7", 0): (43, 3, 3, True, True, 0),
    # ... without the fused automaton the rows of all four fit (one automaton per extraction is smaller than the fused one)
    ("dense_1x13", NO_FUSED): (43, 1, 1, False, False, 4), ("dense_1x14", NO_FUSED): (44, 1, 1, False, False, 4),
    ("dense_2x6", NO_FUSED): (42, 1, 1, False, False, 4), ("dense_2x7", NO_FUSED): (43, 1, 1, False, False, 4),
    ("dense_1x13", RESIDENT): (43, 1, 1, False, False, 4), ("dense_1x14", RESIDENT): (44, 3, 3, True, True, 0),
    ("dense_2x6", RESIDENT): (42, 1, 1, False, False, 4), ("dense_2x7", RESIDENT): (43, 3, 3, True, True, 0),
    # range records: 97 040 bytes of image in LDS at 80 extractions; in global memory from 96 on, while there is a fused automaton
    ("records80", REC): (48, 3, 3, False, False, 4), ("records96", REC): (48, 4, 4, False, False, 4),
    ("wide440", RECG): (48, 4, 4, False, False, 4),
    ("wide_max", REC): (48, 4, 4, False, False, 4), ("wide_max", RECG): (48, 4, 4, False, False, 4),
    ("wide_max+1", RECG): (48, 2, 2, False, False, 4),
    # the fused automaton's last definition and the first without: no hop tables for capture batches (reason 1), two-pass layout
    ("wide_max", 0): (48, 2, 2, True, True, 0), ("wide_max+1", 0): (48, 2, 2, False, True, 1),
    ("states570", 0): (48, 2, 2, False, True, 1), ("states570", L2): (48, 2, 2, False, False, 4),
}


def expected(gorp, name, flags):
    """Assert EXPECT[(name, flags)] on a handle."""
    got = (gorp.stat(1), gorp.stat(7), gorp.stat(9), gorp.stat(14) > 0, gorp.stat(22) > 0, gorp.stat(26))
    assert got == EXPECT[(name, flags)], (name, flags, got, EXPECT[(name, flags)])
