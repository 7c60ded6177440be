"""UTF-8 lines as the Strings Java would see, as far as it goes without a GPU.

The decoding rule (gorp_amd/csrc/gx_utf8.hpp, plain C++) is built with g++ alone into tests/cpp/utf8_test.cpp and compared
with CPython's bytes.decode("utf-8", "replace") -- U+FFFD per maximal subpart -- on every string of up to four bytes over the
alphabet of all boundary bytes, on random longer ones and on well-formed text; the unit -> byte map against the encoder on
well-formed text and against a hand-written table on ill-formed strings.  Then the C ABI: the symbol, the gx_batch_opts layout
(utf8 lies in an older layout's tail padding), and the argument refusals that need no device."""
import ctypes as C
import itertools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = bytes.fromhex("41 7F 80 8F 90 9F A0 BF C0 C1 C2 DF E0 E1 EC ED EE EF F0 F1 F3 F4 F5 FF")


def short_strings():
    """Every string of length 0..4 over ALPHABET (346 201 of them)."""
    out = []
    for k in range(5):
        out.extend(bytes(t) for t in itertools.product(ALPHABET, repeat=k))
    return out


WELL_FORMED = ["", "plain ascii", "caf\u00e9=abc;\u4e2dz", "\u00e9", "\u4e2d", "\U0001F600", "a\U0001F600b\u4e2dc\u00e9d", "\ufeffbom stays",
               "\U0010FFFF\u0800\u07ff\u0080\uffff\U00010000", "x" * 15 + "\u4e2d" + "y" * 14 + "\U0001F600" + "z" * 17 + "\u00e9" * 9]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("utf8") / "utf8_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gorp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "utf8_test.cpp"), "-o", exe])

    def run(strings):
        """-> per string (units as UTF-16-LE bytes, byte index per unit)"""
        blob = b"".join(struct.pack("<I", len(s)) + s for s in strings)
        got = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout
        out, at = [], 0
        for _ in strings:
            (n,) = struct.unpack_from("<I", got, at)
            at += 4
            units = got[at:at + 2 * n]
            at += 2 * n
            where = list(struct.unpack_from("<%dI" % n, got, at))
            at += 4 * n
            out.append((units, where))
        assert at == len(got)
        return out

    return run


def expected_units(s):
    return s.decode("utf-8", "replace").encode("utf-16-le", "surrogatepass")


def test_units_equal_cpython_on_every_short_string(driver):
    strings = short_strings()
    assert len(strings) == sum(24 ** k for k in range(5))
    bad = [s.hex() for s, (units, _) in zip(strings, driver(strings)) if units != expected_units(s)]
    assert not bad, "%d strings differ, e.g. %s" % (len(bad), bad[:5])


def test_units_equal_cpython_on_random_longer_strings(driver):
    rng = random.Random(20260)
    strings = [bytes(rng.choice(ALPHABET) for _ in range(rng.randint(5, 40))) for _ in range(20000)]
    bad = [s.hex() for s, (units, _) in zip(strings, driver(strings)) if units != expected_units(s)]
    assert not bad, "%d strings differ, e.g. %s" % (len(bad), bad[:5])


def test_well_formed_text_units_and_byte_map(driver):
    strings = [t.encode("utf-8") for t in WELL_FORMED]
    for text, s, (units, where) in zip(WELL_FORMED, strings, driver(strings)):
        assert units == text.encode("utf-16-le")
        # unit k starts in the item that begins at the UTF-8 length of the characters before it; the low half of a pair names the pair's
        want, chars = [], 0
        for ch in text:
            at = len(text[:chars].encode("utf-8"))
            want.extend([at] * (2 if ord(ch) > 0xFFFF else 1))
            chars += 1
        assert where == want, text


ILL_FORMED = [
    # bytes, units, byte index per unit
    ("41 E2", [0x41, 0xFFFD], [0, 1]),                                  # truncated lead at the end
    ("E2 82", [0xFFFD], [0]),                                           # ... one maximal subpart of two bytes
    ("F0 9F 98", [0xFFFD], [0]),
    ("E0 80", [0xFFFD, 0xFFFD], [0, 1]),                                # E0 takes A0-BF only
    ("ED A0 80", [0xFFFD, 0xFFFD, 0xFFFD], [0, 1, 2]),                  # an encoded surrogate: three errors
    ("F4 90", [0xFFFD, 0xFFFD], [0, 1]),                                # beyond U+10FFFF
    ("F0 90 80 41", [0xFFFD, 0x41], [0, 3]),                            # a three-byte valid prefix, then ASCII
    ("80 80 BF 41", [0xFFFD, 0xFFFD, 0xFFFD, 0x41], [0, 1, 2, 3]),      # a lone continuation run
    ("41 C3 A9 80 F0 9F 98 80 C0", [0x41, 0xE9, 0xFFFD, 0xD83D, 0xDE00, 0xFFFD], [0, 1, 3, 4, 4, 8]),
]


def test_byte_map_on_ill_formed_strings(driver):
    strings = [bytes.fromhex(h) for h, _, _ in ILL_FORMED]
    for (h, units, where), s, (got_units, got_where) in zip(ILL_FORMED, strings, driver(strings)):
        assert expected_units(s) == np.array(units, "<u2").tobytes(), h   # (the table agrees with CPython)
        assert got_units == np.array(units, "<u2").tobytes(), h
        assert got_where == where, h


def test_lane_logic_of_the_kernel_on_the_cpu(tmp_path):
    """tests/cpp/utf8_lanes_test.cpp: the kernel's per-lane code (window, edge loads, chunk walk, ASCII widening: gx_utf8.hpp) with
    arrays in the place of the shuffles, against the one-thread transcoder -- lines of 0..599 bytes at every alignment."""
    exe = str(tmp_path / "utf8_lanes_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gorp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "utf8_lanes_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "utf8 lanes checks ok" in out.stdout


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def one_rule():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]]])], host_only=True)


def batch_call(g, o):
    data = np.frombuffer(b"abc", dtype=np.uint8)
    offsets = np.array([0, 3], np.uint32)
    mid = np.zeros(1, np.int32)
    caps = np.zeros(2, np.int32)
    return N.lib().gx_extract_batch(g._h.ptr, data.ctypes.data, offsets.ctypes.data, 1, mid.ctypes.data, caps.ctypes.data, C.byref(o))


def test_symbol_and_struct_layout():
    assert "gx_utf8_to_utf16" in N.SYMBOLS
    assert N.lib().gx_utf8_to_utf16.restype is C.c_int
    # utf8 took the previous layout's tail padding: the struct grew by the pointer alone
    assert N.gx_batch_opts.utf8.offset == N.gx_batch_opts.max_line_bytes.offset + 4
    assert N.gx_batch_opts.utf8_line_flags.offset == N.gx_batch_opts.utf8.offset + 4
    assert C.sizeof(N.gx_batch_opts) == N.gx_batch_opts.utf8_line_flags.offset + 8


def test_previous_layout_with_dirty_padding_reads_as_utf8_off():
    """A caller compiled against the layout that ended with max_line_bytes passes that layout's sizeof, whose last four bytes were
    padding: whatever they hold, the call behaves as utf8 = 0 -- here it gets as far as "no device" instead of "bad utf8"."""
    g = one_rule()
    o = N.gx_batch_opts()
    o.struct_size = N.gx_batch_opts.utf8.offset + 4   # sizeof of the previous layout
    o.utf8 = 0xFFFFFFFF
    o.utf8_line_flags = 0xDEADBEEF
    assert batch_call(g, o) == N.GX_E_DEVICE
    assert "no CPU fallback" in N.last_error()
    # the same bytes under the current size are what they say: not a mode
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.utf8_line_flags = None
    assert batch_call(g, o) == N.GX_E_ARG
    assert "utf8" in N.last_error()


def test_refusals_that_need_no_device():
    g = one_rule()
    L = N.lib()

    def opts(**kw):
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    for mode in (1, 2):
        assert batch_call(g, opts(utf8=mode, utf16=1)) == N.GX_E_ARG
        assert "utf16" in N.last_error()
        assert batch_call(g, opts(utf8=mode, device_pointers=1, no_sync=1)) == N.GX_E_ARG
        assert "no_sync" in N.last_error()
    assert batch_call(g, opts(utf8=3)) == N.GX_E_ARG
    # a valid mode gets as far as the missing device: never a CPU path
    assert batch_call(g, opts(utf8=1)) == N.GX_E_DEVICE
    # gx_match_batch
    data = np.frombuffer(b"abc", dtype=np.uint8)
    offsets = np.array([0, 3], np.uint32)
    mid = np.zeros(1, np.int32)
    states = np.zeros(1, np.int32)
    o = opts(utf8=1)
    assert L.gx_match_batch(g._h.ptr, data.ctypes.data, offsets.ctypes.data, 1, mid.ctypes.data, states.ctypes.data, C.byref(o)) == N.GX_E_ARG
    assert "utf8" in N.last_error()
    # the multi-device entry points
    hs = (C.c_void_p * 1)(g._h.ptr)
    caps = np.zeros(2, np.int32)
    assert L.gx_extract_batch_multi(hs, 1, data.ctypes.data, offsets.ctypes.data, 1, mid.ctypes.data, caps.ctypes.data, C.byref(o)) == N.GX_E_ARG
    assert "utf8" in N.last_error()
    shard = N.gx_device_shard(g._h.ptr, None, None, 0, None, None, None, None)
    assert L.gx_extract_batch_multi_device(C.byref(shard), 1, C.byref(o)) == N.GX_E_ARG
    assert "utf8" in N.last_error()
    # gx_utf8_to_utf16: its arguments
    total = C.c_uint64(7)
    o = opts()
    assert L.gx_utf8_to_utf16(data.ctypes.data, None, 1, None, 0, None, C.byref(total), C.byref(o)) == N.GX_E_ARG
    assert L.gx_utf8_to_utf16(data.ctypes.data, offsets.ctypes.data, 1, None, 0, None, None, C.byref(o)) == N.GX_E_ARG
    units = np.zeros(4, np.uint16)
    assert L.gx_utf8_to_utf16(data.ctypes.data, offsets.ctypes.data, 1, units.ctypes.data, 4, None, C.byref(total), C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


def test_python_names_for_the_modes():
    from gorp_amd.gorp import _utf8_mode
    assert [_utf8_mode(v) for v in (None, 0, "bytes", 1, "units", 2)] == [0, 0, 1, 1, 2, 2]
    with pytest.raises(ValueError):
        _utf8_mode("utf-8")
