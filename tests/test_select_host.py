"""The outcome calls (gx_count_outcomes, gx_select_lines, gx_text_select) as far as they go without a GPU: the symbols, the
argument checks, "no device is an error, never a CPU path", and the Python side's outcome index and want masks."""
import ctypes as C

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError

NEW = ["gx_count_outcomes", "gx_select_lines", "gx_text_select"]


def three_rules():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),
                           FlattenedExtraction("beta", [["text", "c"]]),
                           FlattenedExtraction("gamma", [["text", "d"], ["extractor", "y", [["pattern", "\\d+"]]]])], host_only=True)


def opts():
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    return o


def select_args(h, want, offsets, ids, sizes):
    return (h, None, offsets.ctypes.data, len(offsets) - 1, ids.ctypes.data, None, want, None, None, None, None, None, 0, 0,
            C.byref(sizes[0]), C.byref(sizes[1]))


def test_symbols_exported_and_listed():
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int


def test_null_handle_or_null_want_is_an_argument_error():
    L = N.lib()
    g = three_rules()
    o = opts()
    counts = np.zeros(8, np.uint64)
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    want = np.ones(7, np.uint8)
    sizes = (C.c_uint64(0), C.c_uint64(0))
    text = np.frombuffer(b"c\n", dtype=np.uint8)
    calls = [
        lambda: L.gx_count_outcomes(None, ids.ctypes.data, 1, counts.ctypes.data, C.byref(o)),
        lambda: L.gx_count_outcomes(g._h.ptr, ids.ctypes.data, 1, None, C.byref(o)),
        lambda: L.gx_select_lines(*select_args(None, want.ctypes.data, offsets, ids, sizes), C.byref(o)),
        lambda: L.gx_select_lines(*select_args(g._h.ptr, None, offsets, ids, sizes), C.byref(o)),
        lambda: L.gx_text_select(None, text.ctypes.data, 2, want.ctypes.data, None, 0, C.byref(sizes[0]), None, None, C.byref(o)),
        lambda: L.gx_text_select(g._h.ptr, text.ctypes.data, 2, None, None, 0, C.byref(sizes[0]), None, None, C.byref(o)),
    ]
    for call in calls:
        assert call() == N.GX_E_ARG
        assert "bad argument" in N.last_error()


def test_host_only_handle_means_device_error_not_fallback():
    """The rule of test_no_device_means_error_not_fallback: these calls never compute on the CPU."""
    g = three_rules()
    ids = np.array([0, -1, -2], np.int32)
    with pytest.raises(GorpError) as ei:
        g.count_outcomes(ids)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.select_lines(np.frombuffer(b"abczz", dtype=np.uint8), np.array([0, 2, 3, 5], np.uint32), ids, want="unmatched")
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.text_select(b"ab\nc\nzz\n")
    assert ei.value.code == N.GX_E_DEVICE


def test_outcome_index():
    g = three_rules()
    K = 3
    assert g.num_extractions == K
    ids = [K - 1, 0, -1, -2, -1 - K, K, -2 - K, 12345]
    assert g.outcome_index(ids).tolist() == [K - 1, 0, K, K + 1, 2 * K, 2 * K + 1, 2 * K + 1, 2 * K + 1]
    assert [g.outcome_index(v) for v in ids] == g.outcome_index(ids).tolist()
    assert g.outcome_index(-3) == K + 2


def test_want_names_resolve_to_masks():
    g = three_rules()
    #                                                  alpha beta gamma  unmatched  exceptions of alpha, beta, gamma
    assert g.want_mask("unmatched").tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert g.want_mask("exceptions").tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert g.want_mask(["unmatched", "exceptions"]).tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert g.want_mask("beta").tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert g.want_mask(2).tolist() == [0, 0, 1, 0, 0, 0, 0]
    assert g.want_mask(("alpha", 2, "unmatched")).tolist() == [1, 0, 1, 1, 0, 0, 0]
    mask = np.array([1, 0, 0, 0, 0, 0, 1], np.uint8)
    assert g.want_mask(mask).tolist() == mask.tolist()
    assert g.want_mask(bytes(mask)).tolist() == mask.tolist()
    for bad in ("delta", 3, -1, np.zeros(6, np.uint8), ["alpha", "nobody"]):
        with pytest.raises(ValueError):
            g.want_mask(bad)
