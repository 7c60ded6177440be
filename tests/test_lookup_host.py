"""gx_lookup_lines / gx_text_lookup_lines as far as they go without a GPU: the structs against sizeof as the C++ test prints it, the
symbols and the header's text, the Python side's refusals and its reading of `entries` and `keep`, every refusal of the C calls that
needs no device ("no device is an error, never a CPU path" behind them), and the oracle (tests/lookup_oracle.py) on small inputs with
known answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from group_oracle import hash_units
from lookup_oracle import KEEP_HITS, KEEP_OTHERS, MISS, NONE, csr_entries, first_slot, lookup_lines, tag
from test_cpp_lookup_api import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_lookup_lines", "gx_text_lookup_lines"]


def three_rules():
    return Gorp.construct([FlattenedExtraction("alpha", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),
                           FlattenedExtraction("beta", [["text", "c"]]),
                           FlattenedExtraction("gamma", [["text", "d"], ["extractor", "y", [["pattern", "\\d+"]]], ["extractor", "y", [["pattern", "x*"]]],
                                                         ["extractor", "z", [["pattern", "q?"]]]])], host_only=True)


def opts(**kw):
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_struct_layouts_against_sizeof_symbols_and_header_text(tmp_path):
    O, T = N.gx_lookup_out, N.gx_lookup_totals
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    sizes = re.search(r"sizeof gx_lookup_out (\d+) gx_lookup_totals (\d+)", out.stdout)
    assert (C.sizeof(O), C.sizeof(T)) == (int(sizes.group(1)), int(sizes.group(2))) == (96, 80)
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [(name, 8 * q) for q, name in enumerate(
        ("line_entry", "entry_same", "entry_lines", "entry_first_line", "entry_stats", "out_index", "out_bytes", "out_offsets", "out_ids", "out_caps", "cap_lines",
         "out_bytes_cap"))]
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [(name, 8 * q) for q, name in enumerate(
        ("entries", "distinct_entries", "hit_entries", "lines", "keyed", "unset", "hits", "misses", "lines_out", "units_out"))]
    assert (N.GX_LOOKUP_NONE, N.GX_LOOKUP_MISS) == (NONE, MISS) == (0xFFFFFFFF, 0xFFFFFFFE)
    assert (N.GX_LOOKUP_KEEP_NOTHING, N.GX_LOOKUP_KEEP_HITS, N.GX_LOOKUP_KEEP_OTHERS) == (0, KEEP_HITS, KEEP_OTHERS) == (0, 1, 2)
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert len(L.gx_lookup_lines.argtypes) == 18 and len(L.gx_text_lookup_lines.argtypes) == 21
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for struct in (O, T):
        name = struct.__name__
        body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
        at = [re.search(r"[ *,]%s[;,]" % f, body).start() for f, _ in struct._fields_]
        assert at == sorted(at), name
    for text in NEW + ["#define GX_LOOKUP_NONE 0xFFFFFFFFu", "#define GX_LOOKUP_MISS 0xFFFFFFFEu",
                       "enum { GX_LOOKUP_KEEP_NOTHING = 0, GX_LOOKUP_KEEP_HITS = 1, GX_LOOKUP_KEEP_OTHERS = 2 };", "index.putIfAbsent(entry[j], j)",
                       "lines == keyed + unset, keyed == hits + misses", "entry_offsets[0] need not be 0", "SIZE QUERY: out == NULL or every pointer NULL",
                       "EMPTY INPUTS: n == 0, n_parts == 0 and n_entries == 0 are legal", "HOST WAITS: ONE wait", "WORKSPACE: on the handle until gx_destroy"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_lookup.hpp")).read()
    for text in ["GX_WHERE_HD uint32_t lookup_find(", "GX_WHERE_HD uint64_t lookup_word(", "GX_WHERE_HD uint64_t lookup_low_word(", "GX_WHERE_HD bool lookup_keeps("]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule and "atomic" not in rule
    kernels = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_lookup.hip")).read()
    for name in ("k_lookup_build", "k_lookup_probe", "k_lookup_count", "k_lookup_emit", "k_lookup_line_entry"):
        assert "void __launch_bounds__(256) %s(" % name in kernels, name
    assert "gx_lookup.hip" in open(os.path.join(ROOT, "gorp_amd", "build.py")).read()


def test_entries_and_keep_as_the_python_side_reads_them():
    units, offsets = Gorp.lookup_entries([b"ab", "c", b"", "dé"])
    assert units.dtype == np.uint8 and offsets.dtype == np.uint32 and offsets.tolist() == [0, 2, 3, 3, 5] and units.tobytes() == b"abcd\xe9"
    units, offsets = Gorp.lookup_entries(["dé", "€"], encoding="utf-8")
    assert units.tobytes() == "dé€".encode("utf-8") and offsets.tolist() == [0, 3, 6]
    units, offsets = Gorp.lookup_entries(["a１", ""], np.uint16, np.uint64)
    assert units.dtype == np.uint16 and units.tolist() == [0x61, 0xFF11] and offsets.dtype == np.uint64 and offsets.tolist() == [0, 2, 2]
    units, offsets = Gorp.lookup_entries([])
    assert units.size == 0 and offsets.tolist() == [0]
    # a CSR pair and the dict group_lines(..., keys="csr") returns pass through, made of the batch's types
    pair = (np.array([1, 2, 3], np.uint8), np.array([1, 1, 3], np.uint64))
    units, offsets = Gorp.lookup_entries(pair)
    assert offsets.dtype == np.uint32 and offsets.tolist() == [1, 1, 3] and units.tolist() == [1, 2, 3]
    units2, offsets2 = Gorp.lookup_entries({"key_units": pair[0], "key_offsets": pair[1], "lines": None}, np.uint8, np.uint64)
    assert offsets2.dtype == np.uint64 and np.array_equal(units2, units) and csr_entries(units2, offsets2) == [(), (2, 3)]
    with pytest.raises(ValueError):
        Gorp.lookup_entries((np.zeros(3, np.uint8), np.zeros(0, np.uint32)))
    assert [Gorp._lookup_keep(k) for k in (None, False, "hits", "others", 2, 7)] == [0, 0, 1, 2, 2, 7]
    with pytest.raises(ValueError) as ei:
        Gorp._lookup_keep("misses")
    assert "keep" in str(ei.value)


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    return N.gx_group_part(extraction, key_group, value_group, reserved)


def test_refusals_that_need_no_device_and_no_cpu_path_behind_them():
    L = N.lib()
    g = three_rules()
    data = np.frombuffer(b"aXbcd12q", np.uint8).copy()
    offsets = np.array([0, 3, 4, 8], np.uint32)
    ids = np.array([0, 1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    eu = np.frombuffer(b"X12", np.uint8).copy()
    eo = np.array([0, 1, 3], np.uint32)
    room = np.zeros(64, np.uint64)
    tot = N.gx_lookup_totals()

    def call(parts=(part(),), keep=0, flags=0, outputs=(), totals=True, m=2, units=True, entry_offsets=True, rows=True, n=3, cap_lines=8, bytes_cap=64, **kw):
        arr = (N.gx_group_part * max(1, len(parts)))(*parts)
        out = N.gx_lookup_out()
        for name in outputs:
            setattr(out, name, room.ctypes.data)
        out.cap_lines, out.out_bytes_cap = cap_lines, bytes_cap
        rc = L.gx_lookup_lines(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps.ctypes.data if rows else None, arr, len(parts), None, 0,
                               eu.ctypes.data if units else None, eo.ctypes.data if entry_offsets else None, m, keep, flags, C.byref(out),
                               C.byref(tot) if totals else None, C.byref(opts(**kw)))
        return rc, N.last_error()

    refused = [(dict(totals=False), N.GX_E_ARG, "totals is NULL"), (dict(flags=4), N.GX_E_ARG, "unknown flag bits"),
               (dict(parts=[part()] * 65), N.GX_E_LIMIT, "more than 64 parts"), (dict(parts=[part(extraction=3)]), N.GX_E_ARG, "extraction"),
               (dict(parts=[part(extraction=1)]), N.GX_E_ARG, "key_group"), (dict(parts=[part(value_group=1)]), N.GX_E_ARG, "value_group"),
               (dict(parts=[part(reserved=1)]), N.GX_E_ARG, "reserved"), (dict(parts=[part(), part()]), N.GX_E_ARG, "two parts for one extraction"),
               (dict(utf8=2), N.GX_E_ARG, "utf8"), (dict(no_sync=1, device_pointers=1), N.GX_E_ARG, "no_sync"),
               (dict(outputs=("entry_stats",)), N.GX_E_ARG, "entry_stats without a value_group"), (dict(keep=3), N.GX_E_ARG, "keep is not one of"),
               (dict(keep=0, outputs=("out_index",)), N.GX_E_ARG, "GX_LOOKUP_KEEP_NOTHING"), (dict(keep=0, outputs=("out_bytes",)), N.GX_E_ARG, "GX_LOOKUP_KEEP_NOTHING"),
               (dict(keep=1, outputs=("out_caps",), compact_results=2), N.GX_E_ARG, "out_caps on compact rows"),
               (dict(n=2 ** 32 - 1), N.GX_E_LIMIT, "2^32 - 1 lines"), (dict(entry_offsets=False), N.GX_E_ARG, "entry_offsets is NULL"),
               (dict(m=2 ** 30 + 1), N.GX_E_LIMIT, "more than 2^30 entries"), (dict(units=False), N.GX_E_ARG, "entry_units is NULL"),
               (dict(rows=False), N.GX_E_ARG, "need caps"), (dict(compact_results=3), N.GX_E_ARG, "compact_results")]
    for kw, code, words in refused:
        rc, msg = call(**kw)
        assert rc == code and words in msg, (kw, rc, msg)
    # offsets in host memory that go backwards, the batch's and the dictionary's
    eo[1] = 4
    rc, msg = call()
    assert rc == N.GX_E_LIMIT and "entry of 4 G code units" in msg
    eo[1] = 1
    offsets[1] = 5
    rc, msg = call()
    assert rc == N.GX_E_LIMIT and "4 G code units" in msg
    offsets[1] = 3
    # an output on an input or on the dictionary
    out = N.gx_lookup_out()
    for name, target in (("line_entry", ids), ("entry_same", eu), ("entry_lines", eo), ("out_bytes", data)):
        out = N.gx_lookup_out()
        setattr(out, name, target.ctypes.data)
        out.out_bytes_cap = 4
        arr = (N.gx_group_part * 1)(part())
        rc = L.gx_lookup_lines(g._h.ptr, data.ctypes.data, offsets.ctypes.data, 3, ids.ctypes.data, caps.ctypes.data, arr, 1, None, 0, eu.ctypes.data, eo.ctypes.data, 2, 1, 0,
                               C.byref(out), C.byref(tot), C.byref(opts()))
        assert rc == N.GX_E_ARG and "overlaps" in N.last_error(), name
    # ... and behind all of them: no device is an error, never a CPU path.  Among these the size query and the legal empty cases
    fine = [dict(), dict(parts=[]), dict(n=0), dict(m=0, units=False, entry_offsets=False), dict(parts=[], n=0, m=0), dict(keep=1), dict(keep=2),
            dict(keep=1, outputs=("out_index", "out_bytes", "out_offsets", "out_ids", "out_caps")), dict(keep=2, outputs=("out_bytes",), cap_lines=0),
            dict(outputs=("line_entry", "entry_same", "entry_lines", "entry_first_line")), dict(parts=[part(extraction=2, key_group=1, value_group=0)], outputs=("entry_stats",)),
            dict(flags=N.GX_GROUP_WEAK_HASH), dict(utf8=1), dict(utf16=1), dict(compact_results=1), dict(m=2 ** 30, device_pointers=1), dict(offsets64=1, n=0, m=0)]
    for kw in fine:
        rc, msg = call(**kw)
        assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    # the Python wrappers raise the same; what they refuse themselves
    with pytest.raises(GorpError) as ei:
        g.lookup_lines(data, offsets, ids, caps, [("alpha", "x")], [b"X", b"12"], keep="hits")
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_lookup_lines(b"aXb\nc\n", [("alpha", "x")], (eu, eo), keep="others", where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.lookup_lines(data, offsets, ids, caps, [("gamma", "z")], [b"q"], keep=5)
    assert ei.value.code == N.GX_E_ARG
    for bad in (dict(keep="misses"), dict(utf8="units")):
        with pytest.raises(ValueError):
            g.lookup_lines(data, offsets, ids, caps, [("alpha", "x")], [b"X"], **bad)
    with pytest.raises(TypeError):
        g.lookup_lines(data, offsets.astype(np.int64), ids, caps, [("alpha", "x")], [b"X"])
    with pytest.raises(ValueError):
        g.lookup_lines(data, offsets, ids, caps, [("alpha", "x"), ("alpha", "x")], [b"X"])


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_lookup_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_lookup_lines(h, None, off, 1, id_ptr, None, None, 0, None, 0, None, None, 0, 0, 0, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_lookup_lines(None, None, 0, None, 0, None, 0, None, None, 0, 0, 0, None, None, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_lookup_lines(g._h.ptr, None, 5, None, 0, None, 0, None, None, 0, 0, 0, None, None, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    out = N.gx_lookup_out()
    out.out_ids = ids.ctypes.data
    assert L.gx_text_lookup_lines(g._h.ptr, None, 0, None, 0, None, 0, None, None, 0, 1, 0, C.byref(out), None, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert "five batch outputs" in N.last_error()
    assert L.gx_text_lookup_lines(g._h.ptr, None, 0, None, 0, None, 0, None, None, 0, 1, 0, None, None, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_DEVICE


def test_the_oracle_on_a_batch_with_known_answers():
    # a line is its value; caps (0, length); extraction 0 and 1 have parts, line 3 is unmatched, line 5 has no key
    values = [b"bob", b"ann", b"bob", b"eve", b"", b"zed", b"ann"]
    data = np.frombuffer(b"".join(values), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in values])]).astype(np.uint32)
    ids = np.array([0, 1, 0, -1, 1, 0, 1], np.int32)
    caps = np.array([[0, len(v)] for v in values], np.int32)
    caps[5] = [-1, -1]
    entries = [tuple(b"ann"), tuple(b"bob"), tuple(b""), tuple(b"ann"), tuple(b"abe")]
    want = lookup_lines(data, offsets, ids, caps, [(0, 0, -1), (1, 0, -1)], [], 2, entries, KEEP_OTHERS)
    assert want["line_entry"] == [1, 0, 1, NONE, 2, NONE, 0] and want["entry_same"] == [0, 1, 2, 0, 4] and want["entry_lines"] == [2, 2, 1, 0, 0]
    assert want["entry_first_line"] == [1, 0, 4, NONE, NONE] and want["kept"] == [5] and want["entry_stats"] is None
    assert want["totals"] == {"entries": 5, "distinct_entries": 4, "hit_entries": 3, "lines": 6, "keyed": 5, "unset": 1, "hits": 5, "misses": 0, "lines_out": 1,
                              "units_out": 3}
    none = lookup_lines(data, offsets, ids, caps, [(0, 0, 0)], [], 2, [], KEEP_HITS)
    assert none["totals"]["misses"] == 2 and none["totals"]["unset"] == 1 and none["kept"] == [] and none["entry_stats"] == []
    # the hash restated: the first slot and the tag of a text, as the GPU tests choose texts by them
    assert hash_units(b"") >> 64 == 0 and hash_units(b"a") != hash_units(b"b")
    assert first_slot(b"abc", 7) == hash_units(b"abc") & 63 and first_slot(b"abc", 33) == hash_units(b"abc") & 127 and tag(b"abc") == hash_units(b"abc") >> 32
    assert tag(b"abc", weak=True) == 0 and first_slot(b"abc", 1000, weak=True) < 8
