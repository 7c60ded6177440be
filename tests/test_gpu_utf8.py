"""GPU tests of UTF-8 input (gx_batch_opts.utf8, gx_utf8_to_utf16): lines are read as the Strings Java would see.

gx_utf8_to_utf16 is compared with CPython's bytes.decode("utf-8", "replace") -- U+FFFD per maximal subpart, the rule of
gorp_amd/csrc/gx_utf8.hpp -- on the exhaustive short-string set of tests/test_utf8_host.py laid out as adjacent lines without
terminators, so that every ill-formed tail sits against the next line's head.  Extraction is compared with the CPU oracle on
the decoded String, OracleGorp.extract(line.decode("utf-8", "replace")): ids and UTF-16 offsets directly (utf8 = 2), byte
offsets (utf8 = 1) through the unit -> byte map of gx_utf8.hpp as tests/cpp/utf8_test.cpp prints it (checked on the CPU by
test_utf8_host.py).  Everything is compared exactly."""
import ctypes as C
import itertools
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import (FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines, split_lines_device, unpack_rows, utf8_to_utf16,
                           utf8_to_utf16_device)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = bytes.fromhex("41 7F 80 8F 90 9F A0 BF C0 C1 C2 DF E0 E1 EC ED EE EF F0 F1 F3 F4 F5 FF")
E_ACUTE, ZHONG, GRIN = "é".encode(), "中".encode(), "\U0001F600".encode()   # 2, 3 and 4 bytes


def decode(b):
    return bytes(b).decode("utf-8", "replace")


def units_of(b):
    return np.frombuffer(decode(b).encode("utf-16-le", "surrogatepass"), dtype=np.uint16)


def expected_transcode(lines, dtype):
    per = [units_of(ln) for ln in lines]
    off = np.zeros(len(lines) + 1, dtype)
    if lines:
        off[1:] = np.cumsum([len(u) for u in per])
    return (np.concatenate(per) if per else np.zeros(0, np.uint16)), off


def check_transcode(lines, dtype=np.uint32, prefix=b""):
    data, offsets = lines_to_csr(lines, offsets_dtype=dtype)
    if prefix:   # offsets[0] > 0: the batch is a piece of a larger buffer
        data = np.concatenate([np.frombuffer(prefix, dtype=np.uint8), data])
        offsets = (offsets + len(prefix)).astype(dtype)
    units, unit_off = utf8_to_utf16(data, offsets)
    want_units, want_off = expected_transcode(lines, dtype)
    assert unit_off.dtype == dtype and np.array_equal(unit_off, want_off)
    assert np.array_equal(units, want_units)


@pytest.fixture(scope="module")
def short_strings():
    out = []
    for k in range(5):
        out.extend(bytes(t) for t in itertools.product(ALPHABET, repeat=k))
    return out


@pytest.fixture(scope="module")
def byte_map(tmp_path_factory):
    """lines -> per line the byte each unit's item starts at, from gx_utf8.hpp on the CPU (tests/cpp/utf8_test.cpp)."""
    exe = str(tmp_path_factory.mktemp("utf8") / "utf8_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "utf8_test.cpp"), "-o", exe])

    def run(lines):
        blob = b"".join(struct.pack("<I", len(s)) + s for s in lines)
        got = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout
        out, at = [], 0
        for _ in lines:
            (n,) = struct.unpack_from("<I", got, at)
            at += 4 + 2 * n
            out.append(np.frombuffer(got, dtype="<u4", count=n, offset=at).astype(np.int64))
            at += 4 * n
        return out

    return run


# ---------------------------------------------------------------------------
# gx_utf8_to_utf16 vs CPython
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_transcode_every_short_string_as_adjacent_lines(short_strings, dtype):
    assert len(short_strings) == sum(24 ** k for k in range(5))
    check_transcode(short_strings, dtype)


def mixed_line(rng, max_len=90):
    """ASCII with well-formed 2-, 3- and 4-byte characters and some boundary bytes thrown in."""
    out = bytearray()
    for _ in range(rng.randrange(0, max_len)):
        r = rng.random()
        if r < 0.7:
            out.append(rng.randrange(0x20, 0x7F))
        elif r < 0.9:
            out += rng.choice([E_ACUTE, ZHONG, GRIN])
        else:
            out.append(rng.choice(ALPHABET))
    return bytes(out)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049])
def test_transcode_line_counts_at_tile_and_scan_block_edges(n):
    rng = random.Random(100 + n)
    lines = [mixed_line(rng) for _ in range(n)]
    check_transcode(lines, np.uint32, prefix=b"\xf0\x9f")        # (offsets[0] > 0: the batch is a piece of a larger host buffer)
    check_transcode(lines, np.uint64)


def straddling_lines(first_address):
    """Lines laid out from `first_address` (mod 16 is what matters) so that every well-formed and truncated character has each of its
    byte boundaries on a lane's 16-byte chunk boundary, and on the 256-byte boundary between two passes of the line's group (the
    passes start at the line's first byte rounded down to 16)."""
    lines, at = [], first_address
    for ch in (E_ACUTE, ZHONG, GRIN, ZHONG[:2], GRIN[:3], GRIN[:2]):
        for k in range(1, len(ch)):                    # k bytes of the character before the boundary
            for boundary in (16, 32, 256, 512):
                lead = boundary - k - at % 16          # the character starts k bytes before the boundary
                if lead < 0:                           # (the line starts past that point of its first chunk: the next boundary)
                    lead += 16
                ln =b"a" * lead + ch + b"b" * (at % 5)
                lines.append(ln)
                at += len(ln)
    return lines


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_transcode_characters_straddling_every_chunk_boundary(dtype):
    """On device buffers really shifted by 0..15 bytes: a multi-byte character across every 16-byte chunk boundary and across the
    256-byte pass boundary (where the group's edge lanes load their neighbours' bytes themselves), lines starting at every misalignment."""
    import torch
    seen = set()
    for shift in range(16):
        lines = straddling_lines(shift)
        body, offsets = lines_to_csr(lines, offsets_dtype=dtype)
        starts = offsets[:-1].astype(np.int64) + shift
        for ln, st in zip(lines, starts):
            lead = len(ln) - len(ln.lstrip(b"a"))
            seen.add((int(st % 16), int((st % 16 + lead) % 16), (int(st % 16) + lead) // 256))
        buf = np.concatenate([np.full(shift, 0xF0, np.uint8), body, np.full(19, 0x80, np.uint8)])   # (a lead before, continuation bytes behind)
        d = torch.from_numpy(buf).cuda()
        assert d.data_ptr() % 16 == 0
        offsets = (offsets + shift).astype(dtype)
        o = torch.from_numpy(offsets.view(np.int32 if dtype == np.uint32 else np.int64)).cuda()
        want_units, want_off = expected_transcode(lines, dtype)
        n = len(lines)
        units = torch.full((len(want_units) + 32,), 0x5A5A, dtype=torch.int16, device="cuda")
        uoff = torch.zeros(n + 1, dtype=torch.int32 if dtype == np.uint32 else torch.int64, device="cuda")
        total = utf8_to_utf16_device(d.data_ptr(), o.data_ptr(), n, units.data_ptr(), len(want_units), uoff.data_ptr(), offsets64=dtype == np.uint64)
        assert total == len(want_units)
        u = units.cpu().numpy().view(np.uint16)
        assert np.array_equal(u[:total], want_units) and (u[total:] == 0x5A5A).all()
        assert np.array_equal(uoff.cpu().numpy().view(dtype), want_off)
    # the layouts the device saw: every line-start misalignment, and a character start at every chunk position behind a pass boundary
    assert {a for a, _, _ in seen} == set(range(16))
    assert {c for _, c, p in seen if p >= 1} >= {13, 14, 15}


def test_transcode_on_the_device_fenced_sized_and_limited():
    """Device buffers: the bytes just before offsets[0] are a lead and those just behind offsets[n] continuation bytes -- the first
    and last lines must not combine with them; the units buffer is fenced with poison either side; size query; GX_E_LIMIT."""
    import torch
    lines = [GRIN[1:] + b"head", b"plain", ZHONG + b"mid" + E_ACUTE, b"", b"tail" + GRIN[:1]]
    body, offsets = lines_to_csr(lines)
    front = b"\x00" * 13 + GRIN[:1]
    buf = np.concatenate([np.frombuffer(front, np.uint8), body, np.frombuffer(b"\x80\x80\x80" + b"\x00" * 16, np.uint8)])
    offsets = (offsets + len(front)).astype(np.uint32)
    want_units, want_off = expected_transcode(lines, np.uint32)
    assert want_units[0] == 0xFFFD and want_units[-1] == 0xFFFD
    d = torch.from_numpy(buf).cuda()
    o = torch.from_numpy(offsets.view(np.int32)).cuda()
    n = len(lines)
    total = utf8_to_utf16_device(d.data_ptr(), o.data_ptr(), n, None, 0, None)
    assert total == len(want_units)
    FENCE = 64
    units = torch.full((FENCE + total + FENCE,), 0x5A5A, dtype=torch.int16, device="cuda")
    uoff = torch.full((n + 1 + 2,), -7, dtype=torch.int32, device="cuda")
    got = utf8_to_utf16_device(d.data_ptr(), o.data_ptr(), n, units.data_ptr() + 2 * FENCE, total, uoff.data_ptr() + 4)
    assert got == total
    u = units.cpu().numpy().view(np.uint16)
    assert (u[:FENCE] == 0x5A5A).all() and (u[FENCE + total:] == 0x5A5A).all()
    assert np.array_equal(u[FENCE:FENCE + total], want_units)
    uo = uoff.cpu().numpy()
    assert uo[0] == -7 and uo[-1] == -7 and np.array_equal(uo[1:-1].view(np.uint32), want_off)
    # too small: nothing is written, the size is still reported
    units.fill_(0x5A5A)
    opts = N.gx_batch_opts()
    opts.struct_size = C.sizeof(N.gx_batch_opts)
    opts.device_pointers = 1
    size = C.c_uint64(0)
    rc = N.lib().gx_utf8_to_utf16(d.data_ptr(), o.data_ptr(), n, units.data_ptr() + 2 * FENCE, total - 1, uoff.data_ptr() + 4, C.byref(size), C.byref(opts))
    assert rc == N.GX_E_LIMIT and size.value == total
    assert (units.cpu().numpy().view(np.uint16) == 0x5A5A).all()


# ---------------------------------------------------------------------------
# extraction parity with the oracle on the decoded Strings
# ---------------------------------------------------------------------------
def oracle_for(definition):
    built = [e.build() for e in definition]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


# a non-ASCII literal, a counted '.', a non-ASCII class; "caf" is what the first line of the issue matches when read as Latin-1
UNI = [FlattenedExtraction("cafe", [["text", "café="], ["extractor", "three", [["pattern", ".{3}"]]], ["text", ";"], ["extractor", "rest", [["pattern", ".*"]]]]),
       FlattenedExtraction("caf", [["text", "caf"], ["extractor", "all", [["pattern", ".*"]]]]),
       FlattenedExtraction("cls", [["text", "k="], ["extractor", "v", [["pattern", "[é中x]+"]]], ["pattern", " "], ["extractor", "tail", [["pattern", ".*"]]]]),
       FlattenedExtraction("ab", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]])]   # U+2028 inside: the regexp says no


def ascii_word(rng, lo=1, hi=30):
    return bytes(rng.choice(b"abcxyz019_-/.") for _ in range(rng.randrange(lo, hi)))


def uni_lines(n, seed, max_len=None):
    """One line in seven holds a byte >= 0x80: 2-, 3- and 4-byte characters before, inside and after captures; some ill-formed."""
    rng = random.Random(seed)
    special = [
        lambda: "café=abc;中z".encode(),
        lambda: "café=a中c;".encode() + ascii_word(rng) + GRIN + ascii_word(rng),
        lambda: "café=ééé;".encode() + GRIN + E_ACUTE,
        lambda: "café=ab;".encode() + ascii_word(rng),                    # two, not three: falls to "caf"
        lambda: "café=ab\xff;z".encode("latin-1"),                          # U+FFFD is one '.'
        lambda: b"caf" + ascii_word(rng) + ZHONG,
        lambda: b"caf\xc3",                                                      # a truncated lead at the end
        lambda: "k=é中xxé ".encode() + ascii_word(rng) + GRIN,
        lambda: b"k=x\xe4\xb8 " + ascii_word(rng),                               # a truncated character: U+FFFD is not in the class
        lambda: b"k=" + ZHONG * rng.randrange(1, 20) + b" " + E_ACUTE,
        lambda: GRIN + b"caf" + ascii_word(rng),                                 # before everything: no match
        lambda: b"a" + ascii_word(rng) + "\u2028".encode() + b"b",               # automaton yes, regexp no (as a String); Latin-1: a match
        lambda: b"a" + E_ACUTE + ascii_word(rng) + b"b",
        lambda: b"\xed\xa0\x80caf" + ascii_word(rng),
        lambda: ascii_word(rng) + b"\x80\xbf" + ascii_word(rng),
    ]
    plain = [lambda: b"caf" + ascii_word(rng), lambda: b"cafe=abc;" + ascii_word(rng), lambda: b"k=xxx " + ascii_word(rng), lambda: b"a" + ascii_word(rng) + b"b",
             lambda: ascii_word(rng, 0, 60), lambda: b""]
    lines = []
    for i in range(n):
        ln = special[(i // 7) % len(special)]() if i % 7 == 3 else rng.choice(plain)()
        lines.append(ln[:max_len] if max_len else ln)
    return lines


def readme_lines(n, seed):
    rng = random.Random(seed)
    lines = []
    for i in range(n):
        verb = rng.choice(["GET", "PUT", "POST", "HEAD"])
        path = b"/" + ascii_word(rng, 1, 120)
        if i % 7 == 5:
            kind = (i // 7) % 5
            if kind == 0:
                path = b"/" + E_ACUTE + ascii_word(rng) + ZHONG + GRIN
            elif kind == 1:
                path = b"/" + ascii_word(rng) + b"\xe2\x82"                    # ill-formed tail
            elif kind == 2:
                verb = "GÉT"                                               # \w is ASCII: no match
            elif kind == 3:
                path = b"/" + GRIN * rng.randrange(1, 9) + ascii_word(rng)
            else:
                path = b"/a\xffb\xc0" + ascii_word(rng)
        lines.append(b"[%d]: %s %dms %s" % (rng.randrange(10 ** 9), verb.encode(), rng.randrange(5000), path))
    return lines


def oracle_rows(orc, lines, slots):
    ids = np.full(len(lines), -1, np.int32)
    caps = np.full((len(lines), slots), -1, np.int32)
    for i, ln in enumerate(lines):
        k, cp = orc.extract(decode(ln))
        ids[i] = k
        for g, c in enumerate(cp):
            if c is not None:
                caps[i, 2 * g], caps[i, 2 * g + 1] = c
    return ids, caps


def to_byte_offsets(caps_units, lines, where):
    """The oracle's offsets (UTF-16 units of the String) as bytes of the line, through the CPU-tested map."""
    out = caps_units.copy()
    for i, (ln, w) in enumerate(zip(lines, where)):
        table = np.append(w, len(ln))
        sel = caps_units[i] >= 0
        out[i, sel] = table[caps_units[i, sel]]
    return out


def n_flagged(lines):
    return sum(1 for ln in lines if any(b >= 0x80 for b in ln))


SPECIAL = [b"", ZHONG, b"caf" + b"y" * 70000 + ZHONG + b"tail"]   # "", one 3-byte character, a line past 65 535 bytes with a non-ASCII character


@pytest.fixture(scope="module")
def uni_case(byte_map):
    gorp, orc = Gorp.construct(UNI), oracle_for(UNI)
    lines = uni_lines(3000, seed=7) + SPECIAL
    ids, caps = oracle_rows(orc, lines, 2 * gorp.max_groups)
    return gorp, lines, ids, caps, to_byte_offsets(caps, lines, byte_map(lines))


@pytest.fixture(scope="module")
def readme_case(byte_map):
    gorp, orc = Gorp.construct(W.readme3_definition()), oracle_for(W.readme3_definition())
    lines = readme_lines(3000, seed=9) + [b"", ZHONG]
    ids, caps = oracle_rows(orc, lines, 2 * gorp.max_groups)
    return gorp, lines, ids, caps, to_byte_offsets(caps, lines, byte_map(lines))


@pytest.mark.parametrize("which", ["uni", "readme"])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_extraction_equals_the_oracle_on_decoded_strings(which, dtype, uni_case, readme_case):
    gorp, lines, ids, caps_units, caps_bytes = uni_case if which == "uni" else readme_case
    data, offsets = lines_to_csr(lines, offsets_dtype=dtype)
    got_ids, got_caps = gorp.extract_batch(data, offsets, utf8="units")
    assert gorp.stat(33) == n_flagged(lines) and gorp.stat(34) == sum(len(units_of(ln)) for ln in lines if any(b >= 0x80 for b in ln))
    assert np.array_equal(got_ids, ids)
    assert np.array_equal(got_caps, caps_units)
    got_ids, got_caps = gorp.extract_batch(data, offsets, utf8="bytes")
    assert gorp.stat(33) == n_flagged(lines)
    assert np.array_equal(got_ids, ids)
    assert np.array_equal(got_caps, caps_bytes)
    mo_ids, _ = gorp.extract_batch(data, offsets, utf8="bytes", match_only=True)
    assert np.array_equal(mo_ids, np.where(ids < -1, -2 - ids, ids))   # (PolyMatcher.match alone: the automaton's answer)
    if which == "uni":
        # must differ from today: the same bytes read as Latin-1 give other ids (the issue's line: extraction 1 instead of 0)
        old_ids, old_caps = gorp.extract_batch(data, offsets)
        assert (old_ids != ids).any()
        first = lines.index("café=abc;中z".encode())
        assert ids[first] == 0 and caps_units[first].tolist()[:4] == [5, 8, 9, 11] and old_ids[first] == 1 and old_caps[first].tolist()[:2] == [3, 14]
        assert caps_bytes[first].tolist()[:4] == [6, 9, 10, 14]
        # results() materialises the same values from either kind of offsets
        some = [i for i in range(len(lines)) if ids[i] >= 0 and any(b >= 0x80 for b in lines[i])][:50]
        sub = [lines[i] for i in some]
        sd, so = lines_to_csr(sub)
        by_units = gorp.results(sd, so, ids[some], caps_units[some], utf8="units")
        by_bytes = gorp.results(sd, so, ids[some], caps_bytes[some], utf8="bytes")
        assert [r.asMap() for r in by_units] == [r.asMap() for r in by_bytes]
        assert by_bytes[0].getInput() == decode(sub[0])


@pytest.mark.parametrize("compact,kernel", [(1, N.GX_KERNEL_AUTO), (2, N.GX_KERNEL_TILES), (0, N.GX_KERNEL_PER_LINE), (1, N.GX_KERNEL_TILES)])
@pytest.mark.parametrize("mode", ["bytes", "units"])
def test_row_formats_and_named_kernels(compact, kernel, mode, byte_map):
    gorp, orc = Gorp.construct(UNI), oracle_for(UNI)
    lines = uni_lines(1500, seed=21 + compact, max_len=250 if compact == 2 else None)   # (u8 rows: lines under 255 bytes)
    ids, caps = oracle_rows(orc, lines, 2 * gorp.max_groups)
    want = caps if mode == "units" else to_byte_offsets(caps, lines, byte_map(lines))
    data, offsets = lines_to_csr(lines)
    if compact:
        rows, over = gorp.extract_batch(data, offsets, utf8=mode, compact=compact, kernel=kernel)
        got_ids, got_caps = unpack_rows(rows)
        assert over == 0
    else:
        got_ids, got_caps = gorp.extract_batch(data, offsets, utf8=mode, kernel=kernel)
    assert gorp.stat(33) == n_flagged(lines)
    assert np.array_equal(got_ids, ids) and np.array_equal(got_caps, want)


def test_u16_rows_count_the_offsets_of_a_long_line_that_do_not_fit(byte_map):
    gorp = Gorp.construct(UNI)
    lines = [b"caf" + b"y" * 70000 + ZHONG + b"tail", b"caf" + ZHONG]
    data, offsets = lines_to_csr(lines)
    rows, over = gorp.extract_batch(data, offsets, utf8="bytes", compact=1)
    ids, caps = unpack_rows(rows)
    assert ids.tolist() == [1, 1] and caps[0].tolist()[:2] == [3, 65534] and caps[1].tolist()[:2] == [3, 6]
    assert gorp.stat(33) == 2
    assert over >= 1   # (a line that is walked again counts its clipped offsets more than once: include/gorp_hip.h)


@pytest.mark.parametrize("compact", [0, 1])
def test_device_pointers_strip_eol_and_flags_from_the_split_pass(compact, byte_map):
    """Raw text with all three terminators -> gx_split_lines (offsets and line flags on the device) -> gx_extract_batch with
    strip_eol, 64-bit offsets and the split pass's flags in place of the sweep."""
    import torch
    gorp, orc = Gorp.construct(UNI), oracle_for(UNI)
    rng = random.Random(33)
    lines = uni_lines(3000, seed=31)
    text = b"".join(ln + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in lines[:-1]) + lines[-1]   # (the last line needs no terminator)
    _, kept, flags = O.read_lines(text)
    lines = kept
    ids, caps = oracle_rows(orc, lines, 2 * gorp.max_groups)
    caps_bytes = to_byte_offsets(caps, lines, byte_map(lines))
    n = len(lines)
    d = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert split_lines_device(d.data_ptr(), len(text), off.data_ptr(), n, flags_ptr=fl.data_ptr(), offsets64=True) == n
    assert np.array_equal(fl.cpu().numpy(), flags)
    slots = 2 * gorp.max_groups
    for mode, want in ((1, caps_bytes), (2, caps)):
        for flags_ptr in (fl.data_ptr(), None):
            if compact:
                rows = torch.zeros((n, 1 + slots), dtype=torch.int16, device="cuda")
                over = torch.zeros(1, dtype=torch.int64, device="cuda")
                gorp.extract_batch_device(d.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), offsets64=True, strip_eol=True, compact=1,
                                          overflow_ptr=over.data_ptr(), utf8=mode, utf8_line_flags_ptr=flags_ptr)
                got_ids, got_caps = unpack_rows(rows.cpu().numpy())
                assert int(over[0]) == 0
            else:
                mid = torch.zeros(n, dtype=torch.int32, device="cuda")
                cp = torch.zeros((n, slots), dtype=torch.int32, device="cuda")
                gorp.extract_batch_device(d.data_ptr(), off.data_ptr(), n, mid.data_ptr(), cp.data_ptr(), offsets64=True, strip_eol=True,
                                          utf8=mode, utf8_line_flags_ptr=flags_ptr)
                got_ids, got_caps = mid.cpu().numpy(), cp.cpu().numpy()
            assert gorp.stat(33) == int(flags.sum())
            assert np.array_equal(got_ids, ids) and np.array_equal(got_caps, want)


def test_host_pointers_with_line_flags_from_split_lines(byte_map):
    """Host buffers all the way: split_lines(want_flags=True) -> extract_batch(strip_eol, utf8, utf8_line_flags): the flags are staged
    with the batch and take the sweep's place."""
    gorp, orc = Gorp.construct(UNI), oracle_for(UNI)
    lines = uni_lines(700, seed=51)
    text = b"".join(ln + b"\n" for ln in lines)
    offsets, flags = split_lines(text, want_flags=True)
    assert len(flags) == len(lines) and int(flags.sum()) == n_flagged(lines)
    ids, caps = oracle_rows(orc, lines, 2 * gorp.max_groups)
    data = np.frombuffer(text, np.uint8)
    got_ids, got_caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="units", utf8_line_flags=flags)
    assert gorp.stat(33) == n_flagged(lines)
    assert np.array_equal(got_ids, ids) and np.array_equal(got_caps, caps)
    got_ids, got_caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes", utf8_line_flags=flags)
    assert np.array_equal(got_ids, ids) and np.array_equal(got_caps, to_byte_offsets(caps, lines, byte_map(lines)))
    # the flags are believed: a line flagged 0 is read as Latin-1 (include/gorp_hip.h)
    none = np.zeros_like(flags)
    lat_ids, _ = gorp.extract_batch(data, offsets, strip_eol=True, utf8="units", utf8_line_flags=none)
    assert gorp.stat(33) == 0 and np.array_equal(lat_ids, gorp.extract_batch(data, offsets, strip_eol=True)[0])


def test_all_ascii_batch_is_the_byte_path_untouched():
    gorp = Gorp.construct(W.readme3_definition())
    data, offsets, _ = W.readme3_lines(4000, seed=5)
    d, o = data.numpy(), offsets.numpy().astype(np.uint32)
    want = gorp.extract_batch(d, o)
    for mode in ("bytes", "units"):
        got = gorp.extract_batch(d, o, utf8=mode)
        assert gorp.stat(33) == 0 and gorp.stat(34) == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_refusals_on_the_device():
    import torch
    gorp = Gorp.construct(UNI)
    data, offsets = lines_to_csr([b"caf", b"k=x y"])
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(offsets.view(np.int32)).cuda()
    mid = torch.zeros(2, dtype=torch.int32, device="cuda")
    cp = torch.zeros((2, 2 * gorp.max_groups), dtype=torch.int32, device="cuda")
    for kw in ({"no_sync": True}, {"utf16": True}):
        with pytest.raises(GorpError) as ei:
            gorp.extract_batch_device(d.data_ptr(), o.data_ptr(), 2, mid.data_ptr(), cp.data_ptr(), utf8=1, **kw)
        assert ei.value.code == N.GX_E_ARG
    opts = N.gx_batch_opts()
    opts.struct_size = C.sizeof(N.gx_batch_opts)
    opts.utf8 = 1
    hs = (C.c_void_p * 1)(gorp._h.ptr)
    m = np.zeros(2, np.int32)
    c = np.zeros((2, 2 * gorp.max_groups), np.int32)
    assert N.lib().gx_extract_batch_multi(hs, 1, data.ctypes.data, offsets.ctypes.data, 2, m.ctypes.data, c.ctypes.data, C.byref(opts)) == N.GX_E_ARG
    shard = N.gx_device_shard(gorp._h.ptr, d.data_ptr(), o.data_ptr(), 2, mid.data_ptr(), cp.data_ptr(), None, None)
    assert N.lib().gx_extract_batch_multi_device(C.byref(shard), 1, C.byref(opts)) == N.GX_E_ARG
    assert "utf8" in N.last_error()


# ---------------------------------------------------------------------------
# whole files: gx_text_to_jsonl(utf8), gx_text_select(utf8)
# ---------------------------------------------------------------------------
def well_formed_text(n, seed):
    rng = random.Random(seed)
    lines = [ln for ln in uni_lines(2 * n, seed) if decode(ln).encode("utf-8") == ln][:n]
    assert len(lines) == n and n_flagged(lines) > n // 20
    return lines, b"".join(ln + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in lines)


def test_text_to_jsonl_and_text_select_on_utf8_text():
    gorp, orc = Gorp.construct(UNI), oracle_for(UNI)
    _, text = well_formed_text(2000, seed=41)
    off, lines, flags = O.read_lines(text)
    xs = gorp.getExtractions()
    want_objs, dead = [], bytearray()
    n_matched = n_exc = 0
    for i, ln in enumerate(lines):
        s = decode(ln)
        k, cp = orc.extract(s)
        if k < 0:
            dead += text[int(off[i]):int(off[i + 1])]
            n_exc += k < -1
            continue
        n_matched += 1
        units = s.encode("utf-16-le", "surrogatepass")
        m = {"rule": xs[k].getName()}
        for name, c in zip(xs[k]._extractorNames, cp):
            m[name] = None if c is None else units[2 * c[0]:2 * c[1]].decode("utf-16-le", "surrogatepass")
        want_objs.append(m)
    assert n_exc > 0 and n_matched > 500
    out, nl, nm, nx = gorp.text_to_jsonl(text, id_as="rule", utf8=True)
    assert gorp.stat(33) == int(flags.sum())
    assert (nl, nm, nx) == (len(lines), n_matched, n_exc)
    got_objs = [json.loads(t) for t in out.decode("utf-8").split("\n")[:-1]]
    assert got_objs == want_objs
    # read as Latin-1 the same text gives other answers: the option is what makes the difference
    assert gorp.text_to_jsonl(text, id_as="rule", utf8_passthrough=True)[0] != out
    K = gorp.num_extractions
    sel, counts, n_lines = gorp.text_select(text, utf8=True)
    assert gorp.stat(33) == int(flags.sum())
    assert n_lines == len(lines) and sel == bytes(dead)
    assert int(counts[:K].sum()) == n_matched and int(counts[K + 1:2 * K + 1].sum()) == n_exc and int(counts[K]) == len(lines) - n_matched - n_exc


def test_byte_offsets_compose_with_results_to_jsonl_passthrough():
    gorp = Gorp.construct(UNI)
    lines, _ = well_formed_text(1500, seed=43)
    data, offsets = lines_to_csr(lines)
    ids, caps = gorp.extract_batch(data, offsets, utf8="bytes")
    assert gorp.stat(33) == n_flagged(lines)
    composed = gorp.results_to_jsonl(data, offsets, ids, caps, id_as="rule", utf8_passthrough=True)
    whole, _, nm, _ = gorp.text_to_jsonl(b"".join(ln + b"\n" for ln in lines), id_as="rule", utf8=True)
    assert nm == int((ids >= 0).sum()) > 300
    assert composed == whole
