"""The partition calls (gx_partition_lines, gx_text_to_jsonl_by_extraction) as far as they go without a GPU: the symbols, the
argument checks, "no device is an error, never a CPU path", and the Python side's plumbing of want=None."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError

NEW = ["gx_partition_lines", "gx_text_to_jsonl_by_extraction"]


def three_rules():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),
                           FlattenedExtraction("beta", [["text", "c"]]),
                           FlattenedExtraction("gamma", [["text", "d"], ["extractor", "y", [["pattern", "\\d+"]]]])], host_only=True)


def opts():
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    return o


def partition_args(h, offsets, ids, sizes):
    return (h, None, offsets, 1, ids.ctypes.data, None, None, None, None, None, None, None, 0, 0, None, None, sizes[0], sizes[1])


def test_symbols_exported_and_listed():
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int


def test_header_declares_them():
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(N.__file__)), "..", "include", "gorp_hip.h")).read()
    for name in NEW:
        assert "int %s(gx_handle* h" % name in header


def test_null_handle_offsets_or_sizes_is_an_argument_error():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    sizes = (C.c_uint64(0), C.c_uint64(0))
    both = (C.byref(sizes[0]), C.byref(sizes[1]))
    text = np.frombuffer(b"c\n", dtype=np.uint8)
    calls = [
        lambda: L.gx_partition_lines(*partition_args(None, offsets.ctypes.data, ids, both), C.byref(o)),
        lambda: L.gx_partition_lines(*partition_args(g._h.ptr, None, ids, both), C.byref(o)),
        lambda: L.gx_partition_lines(*partition_args(g._h.ptr, offsets.ctypes.data, ids, (None, both[1])), C.byref(o)),
        lambda: L.gx_partition_lines(*partition_args(g._h.ptr, offsets.ctypes.data, ids, (both[0], None)), C.byref(o)),
        lambda: L.gx_text_to_jsonl_by_extraction(None, text.ctypes.data, 2, None, None, 0, both[0], None, None, None, C.byref(o)),
        lambda: L.gx_text_to_jsonl_by_extraction(g._h.ptr, text.ctypes.data, 2, None, None, 0, None, None, None, None, C.byref(o)),
        lambda: L.gx_text_to_jsonl_by_extraction(g._h.ptr, None, 2, None, None, 0, both[0], None, None, None, C.byref(o)),
    ]
    for call in calls:
        assert call() == N.GX_E_ARG
        assert "bad argument" in N.last_error()


def test_host_only_handle_means_device_error_not_fallback():
    """The rule of test_no_device_means_error_not_fallback: these calls never compute on the CPU."""
    g = three_rules()
    ids = np.array([0, -1, -2], np.int32)
    data, offsets = np.frombuffer(b"abczz", dtype=np.uint8), np.array([0, 2, 3, 5], np.uint32)
    for want in (None, "unmatched"):
        with pytest.raises(GorpError) as ei:
            g.partition_lines(data, offsets, ids, want=want)
        assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_to_jsonl_by_extraction(b"ab\nc\nzz\n", id_as="rule")
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message


def test_want_none_reaches_the_library_as_null(monkeypatch):
    """want=None is "every outcome 0 .. 2K": the C ABI's NULL, not a mask made up in Python; a named want is its want_mask."""
    g = three_rules()
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def gx_partition_lines(self, *args):
            seen.append(None if args[6] is None else bytes((C.c_uint8 * 7).from_address(args[6])))
            return real.gx_partition_lines(*args)

    real = N.lib()
    monkeypatch.setattr(N, "lib", lambda: Spy())
    for want in (None, ["beta", "unmatched"]):
        with pytest.raises(GorpError):
            g.partition_lines_device(None, 0x1000, 0, None, None, want)
    assert seen[0] is None
    mask = g.want_mask(["beta", "unmatched"])
    assert seen[1] == bytes(mask) == bytes([0, 1, 0, 1, 0, 0, 0])
    with pytest.raises(ValueError):
        g.partition_lines_device(None, 0x1000, 0, None, None, "nobody")
