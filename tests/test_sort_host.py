"""gx_sort_lines / gx_text_sort_lines as far as they go without a GPU: the symbols and struct layouts, every refusal that needs no
device and "no device is an error, never a CPU path" behind them, the Python wrappers, and the rule itself --
gorp_amd/csrc/gx_sort.hpp, plain C++ -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into
tests/cpp/sort_test.cpp and run as a program of its own: the digit plan, the class rule, the places and a host replay of the plan's
passes, against sorted() (tests/sort_oracle.py).  The numpy restatement the large GPU case is compared with equals the oracle on every
small draw."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from sort_oracle import CARRIED, REST, STAMPED, classes, key_of, np_sort, order_of, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_sort_lines", "gx_text_sort_lines"]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


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


def test_symbols_struct_layouts_and_header_text():
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    a = L.gx_sort_lines.argtypes
    assert len(a) == 14 and a[6] == C.POINTER(N.gx_top_part) and a[8] == C.POINTER(N.gx_where_term) and a[10] is C.c_uint32
    assert a[11] == C.POINTER(N.gx_sort_out) and a[12] == C.POINTER(N.gx_sort_totals) and a[13] == C.POINTER(N.gx_batch_opts)
    t = L.gx_text_sort_lines.argtypes
    assert len(t) == 18 and t[3] == C.POINTER(N.gx_top_part) and t[7] is C.c_uint32 and t[9] is C.c_uint64 and t[14] == C.POINTER(N.gx_sort_totals)
    # the layouts of include/gorp_hip.h: nine 8-byte fields; ten 8-byte fields and two of 4 bytes
    assert C.sizeof(N.gx_sort_out) == 72 and [(f[0], getattr(N.gx_sort_out, f[0]).offset) for f in N.gx_sort_out._fields_] == [
        ("out_index", 0), ("out_values", 8), ("out_class", 16), ("out_bytes", 24), ("out_offsets", 32), ("out_ids", 40), ("out_caps", 48), ("cap_lines", 56),
        ("out_bytes_cap", 64)]
    assert C.sizeof(N.gx_sort_totals) == 88 and [(f[0], getattr(N.gx_sort_totals, f[0]).offset) for f in N.gx_sort_totals._fields_] == [
        ("lines", 0), ("numbers", 8), ("unset", 16), ("not_numbers", 24), ("carried", 32), ("rest", 40), ("lines_out", 48), ("units_out", 56), ("first_value", 64),
        ("last_value", 72), ("n_passes", 80), ("already_ordered", 84)]
    assert (N.GX_SORT_DESCENDING, N.GX_SORT_CARRY, N.GX_SORT_REST_LAST, N.GX_SORT_ALL_DIGITS) == (1, 2, 4, 8)
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["#define GX_SORT_DESCENDING 1u", "#define GX_SORT_CARRY      2u", "#define GX_SORT_REST_LAST  4u", "#define GX_SORT_ALL_DIGITS 8u",
                       "typedef struct gx_sort_out {", "typedef struct gx_sort_totals {", "Comparator.comparingLong", "README.md:26,63-79",
                       "nearest earlier", "ONE host wait before any output", "50 bytes per INPUT line", "may now lie in the middle",
                       "an output overlapping an input", "out_caps on compact rows", "n above 2^30", "copies the batch through"]:
        assert text in header, text
    mirror = open(os.path.join(ROOT, "include", "gorp.hpp")).read()
    assert "sortLines(" in mirror and "textSortLines(" in mirror
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_sort.hpp")).read()
    # reused, not copied
    assert "hip_runtime" not in rule and "bucket_digit(" in rule and "gq_lower_bound(" in rule and "GQ_VALUE_DIGITS" in rule
    for copied in ("uint64_t top_key", "int64_t top_value", "uint32_t bucket_digit", "uint32_t GQ_DIGIT_BITS", "uint64_t gq_lower_bound"):
        assert copied not in rule, copied
    kernels = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_sort.hip")).read()
    assert '#include "gx_bucket_sort_dev.hpp"' in kernels and "launch_top_keys(" in kernels and "atomic" not in kernels.split("#include", 1)[1]


def part(extraction=0, value_group=0):
    p = N.gx_top_part()
    p.extraction, p.value_group = extraction, value_group
    return p


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


def test_every_refusal_comes_before_the_look_at_the_device():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8).copy()
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8).copy()
    totals = N.gx_sort_totals()
    o_index, o_values, o_class = np.zeros(8, np.uint32), np.zeros(8, np.int64), np.zeros(8, np.uint8)
    o_bytes, o_off, o_ids, o_caps = np.zeros(64, np.uint8), np.zeros(9, np.uint32), np.zeros(64, np.int32), np.zeros((8, 6), np.int32)

    def full_out(**kw):
        b = N.gx_sort_out(o_index.ctypes.data, o_values.ctypes.data, o_class.ctypes.data, o_bytes.ctypes.data, o_off.ctypes.data, o_ids.ctypes.data,
                          o_caps.ctypes.data, 8, 64)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def both(parts, n_parts=None, terms=(), n_terms=None, caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals), n=3, off=offsets, flags=0, out=None, ids_arr=ids,
             **kw):
        arr = None
        if parts is not None:
            arr = (N.gx_top_part * max(1, len(parts)))()
            for i, p in enumerate(parts):
                arr[i] = p
        n_parts = len(parts) if n_parts is None else n_parts
        tarr = None
        if terms is not None:
            tarr = (N.gx_where_term * max(1, len(terms)))()
            for i, t in enumerate(terms):
                tarr[i] = t
        n_terms = len(terms) if n_terms is None else n_terms
        o = opts(**kw)
        b = out if out is not None else N.gx_sort_out()
        rc1 = L.gx_sort_lines(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids_arr.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, flags,
                              None if out is None else C.byref(b), totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_sort_lines(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, flags, b.out_bytes, b.out_bytes_cap, b.out_offsets,
                                   b.out_index, b.out_values, b.out_class, totals_ptr, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    # in the order the call makes them: totals, the flags, the parts, utf8 = 2, the terms, no_sync
    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None), dict(parts=[part()] * 65, totals_ptr=None),       # totals == NULL, before everything
        dict(parts=[part()], flags=16), dict(parts=[], flags=0x80000000), dict(parts=[part()], flags=1 | 2 | 4 | 8 | 32), dict(parts=[part()] * 65, flags=16),
        dict(parts=None, n_parts=1),                                                  # gx_top_lines' refusals of the parts ...
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(2, 3)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2), dict(parts=[part()], utf8=2, terms=[term()] * 65),
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),   # ... of the terms
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    # out_caps on compact rows; out_caps without caps; an output that overlaps an input (the batch call: the text call has neither)
    rows16 = np.zeros((3, 7), np.uint16)
    for kw, word in ((dict(parts=[part()], out=full_out(), compact_results=1, ids_arr=rows16), "compact rows"),
                     (dict(parts=[], out=full_out(), caps_ptr=None), "out_caps without caps"),
                     (dict(parts=[part()], out=full_out(out_bytes=data.ctypes.data + 3)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_index=offsets.ctypes.data)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_values=ids.ctypes.data + 8)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_class=data.ctypes.data + 6)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_ids=ids.ctypes.data + 8)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_offsets=caps.ctypes.data + 4)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_caps=offsets.ctypes.data - 16)), "overlaps"),
                     # a capacity that means "large enough" loses no refusal: no product of it wraps to nothing
                     (dict(parts=[part()], out=full_out(out_index=offsets.ctypes.data, cap_lines=2 ** 64 - 1)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_values=ids.ctypes.data - 8, cap_lines=2 ** 62)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_ids=caps.ctypes.data, cap_lines=2 ** 63)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_bytes=data.ctypes.data - 8, out_bytes_cap=2 ** 64 - 1)), "overlaps")):
        (rc, msg), _ = both(**kw)
        assert rc == N.GX_E_ARG and word in msg, (word, rc, msg)
    for out in (full_out(out_bytes=text.ctypes.data + 8), full_out(out_values=text.ctypes.data - 4), full_out(out_class=text.ctypes.data + 1)):
        _, (rc, msg) = both(parts=[part()], out=out)
        assert rc == N.GX_E_ARG and "overlaps" in msg
    # the class bytes right behind the text do not overlap it
    _, (rc, msg) = both(parts=[part()], out=full_out(out_class=text.ctypes.data + len(text)))
    assert rc == N.GX_E_DEVICE
    limit = [
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT and "64" in msg, (kw, msg)
            assert "no CPU fallback" not in msg
    # n above 2^30, with host buffers and with device pointers; a line of 2^32 units or more, and offsets that go backwards (host offsets)
    for kw in (dict(n=2 ** 30 + 1, device_pointers=1), dict(n=2 ** 32, device_pointers=1), dict(n=2 ** 30 + 1, device_pointers=1, out=full_out())):
        (rc, msg), _ = both(parts=[part()], **kw)
        assert rc == N.GX_E_LIMIT and "2^30" in msg
    for off in (np.array([0, 2, 5, 5 + 2 ** 32], np.uint64), np.array([0, 2, 1, 7], np.uint64)):
        (rc, msg), _ = both(parts=[part()], off=off, offsets64=1)
        assert rc == N.GX_E_LIMIT and "4 G code units" in msg
    # parts or terms on dense ids without caps (the whole-file call makes its own)
    for kw in (dict(parts=[part()]), dict(parts=[], terms=[term()])):
        (rc, msg), (rc2, msg2) = both(caps_ptr=None, **kw)
        assert rc == N.GX_E_ARG and "caps" in msg
        assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part(2, 2), part()]), dict(parts=[part()], out=full_out()), dict(parts=[], out=full_out()),
            dict(parts=[], caps_ptr=None), dict(parts=[], n=0),
            dict(parts=[part()], flags=N.GX_SORT_DESCENDING), dict(parts=[part()], flags=N.GX_SORT_CARRY), dict(parts=[part()], flags=N.GX_SORT_REST_LAST),
            dict(parts=[part()], flags=N.GX_SORT_ALL_DIGITS), dict(parts=[part()], flags=15, out=full_out()),
            dict(parts=[part(2, 0), part()], terms=[term()] * 64), dict(parts=[part()], utf8=1),
            dict(parts=[part()], compact_results=2, ids_arr=np.zeros((3, 7), np.uint8)),
            dict(parts=[part()], compact_results=1, ids_arr=rows16, out=full_out(out_caps=None)),
            dict(parts=[part()], n=2 ** 30, device_pointers=1)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.sort_lines(data, offsets, ids, caps, [("alpha", "x")], carry=True, rest="last")
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_sort_lines(bytes(text), [("gamma", "z")], descending=True, where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.sort_lines(data, offsets, ids, None, [("alpha", "x")])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(ValueError):
        g.sort_lines(data, offsets, ids, caps, [("alpha", "x")], rest="first")
    with pytest.raises(ValueError):
        g.sort_lines(data, offsets, ids, caps, [("alpha", "x")], utf8="units")
    with pytest.raises(ValueError):
        g.sort_lines(data, offsets, ids, caps, [("alpha", "nope")])
    assert Gorp._sort_flags(True, True, "last", True) == 15 and Gorp._sort_flags(False, False, "drop", False) == 0 and Gorp._sort_flags(False, True, "drop", False) == 2


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_sort_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_sort_lines(h, None, off, 1, id_ptr, None, None, 0, None, 0, 0, None, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    args = (None, 0, None, 0, 0, None, 0, None, None, None, None, C.byref(t), None, None, C.byref(o))
    assert L.gx_text_sort_lines(None, None, 0, *args) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_sort_lines(g._h.ptr, None, 5, *args) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sort") / "sort_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sort_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def test_the_digit_plan(rule_exe):
    base = key_of(1234567890123)
    sets = {"none": [], "one": [base], "all equal": [base] * 5, "min and max": [key_of(INT64_MIN), key_of(INT64_MAX)]}
    for bit in (0, 5, 6, 59, 60, 63):
        sets["bit %d" % bit] = [base, base ^ (1 << bit), base]
    by_hand = {"none": [], "one": [], "all equal": [], "min and max": list(range(11)), "bit 0": [0], "bit 5": [0], "bit 6": [1], "bit 59": [9], "bit 60": [10],
               "bit 63": [10]}
    assert key_of(INT64_MIN) == 0 and key_of(INT64_MAX) == 2 ** 64 - 1 and key_of(INT64_MIN, True) == 2 ** 64 - 1 and key_of(-1) + 1 == key_of(0)
    cases = [(name, a) for name in sets for a in (0, 1)]
    rows = ["P %d %d %s" % (a, len(sets[name]), " ".join("%x" % k for k in sets[name])) for name, a in cases]
    for (name, a), line in zip(cases, run_cases(rule_exe, rows)):
        nums = [int(x) for x in line.split()]
        want = plan(sets[name], bool(a))
        assert a or want == by_hand[name], name
        assert not a or want == (list(range(11)) if sets[name] else []), name
        assert nums[0] == len(want) and nums[1] == len(want) % 2 and nums[2:] == want, (name, a, nums)


def replay(exe, cases):
    """cases: (values per line -- int or None --, descending, carry, rest_last, all_digits); the program's rows as dicts"""
    rows = ["S %d %d %d %d %d %s" % (d, c, r, a, len(v), " ".join("x" if x is None else str(x) for x in v)) for v, d, c, r, a in cases]
    out = []
    for line in run_cases(exe, rows):
        nums = [int(x) for x in line.split()]
        head, body = nums[:8], nums[8:]
        out.append({"m": head[0], "carried": head[1], "rest": head[2], "leading": head[3], "n_passes": head[4], "already_ordered": head[5], "first": head[6],
                    "last": head[7], "index": body[0::3], "values": body[1::3], "classes": body[2::3]})
    return out


def check_replay(exe, cases):
    for (values, d, c, r, a), got in zip(cases, replay(exe, cases)):
        index, out_values, out_class, carried, rest = order_of(values, bool(c), bool(d), bool(r))
        what = (values[:12], d, c, r, a)
        m = len([x for x in out_class if x != REST])
        assert got["index"] == index and got["values"] == out_values and got["classes"] == out_class, what
        assert (got["m"], got["carried"], got["rest"]) == (m, carried, rest), what
        assert got["leading"] == next((i for i, v in enumerate(values) if v is not None), len(values)), what
        keys = [key_of(v, bool(d)) for v in out_values[:m]]
        assert got["n_passes"] == len(plan(keys, bool(a))), what
        assert (got["first"], got["last"]) == ((out_values[0], out_values[m - 1]) if m else (0, 0)), what
        stamped = [key_of(v, bool(d)) for v in values if v is not None]
        assert got["already_ordered"] == int(all(x <= y for x, y in zip(stamped, stamped[1:]))), what


def test_the_replay_of_the_plans_passes_equals_sorted_in_both_directions(rule_exe):
    rng = random.Random(17)
    draws = [[rng.randrange(-50, 50) for _ in range(300)], [rng.randrange(INT64_MIN, INT64_MAX + 1) for _ in range(200)],
             [rng.choice([INT64_MIN, INT64_MAX, 0, -1]) for _ in range(100)], [7] * 70, [rng.randrange(0, 7) for _ in range(500)],
             [(rng.randrange(0, 64) << 30) | 5 for _ in range(150)], list(range(100)), list(range(100, 0, -1)),
             [x for pair in zip(range(0, 200, 2), range(1, 201, 2)) for x in pair][:150] + list(range(50, 120)), [], [3]]
    cases = [(v, d, 0, 0, a) for v in draws for d in (0, 1) for a in (0, 1)]
    check_replay(rule_exe, cases)
    # by hand: ascending by (value, line), descending by (-value, line) -- ties keep their input order in both
    (up, down) = replay(rule_exe, [([5, 3, 5, 3], 0, 0, 0, 0), ([5, 3, 5, 3], 1, 0, 0, 0)])
    assert up["index"] == [1, 3, 0, 2] and down["index"] == [0, 2, 1, 3] and up["n_passes"] == 1 and up["already_ordered"] == 0


def test_the_carry_rule(rule_exe):
    rng = random.Random(23)
    shapes = {"no stamped line": [None] * 9, "a stamped line first": [4] + [None] * 6, "a stamped line last": [None] * 6 + [4],
              "alternating": [v for i in range(20) for v in (20 - i, None)], "alternating, unstamped first": [v for i in range(20) for v in (None, i % 3)],
              "records": [v for i in range(60) for v in [rng.randrange(0, 9)] + [None] * rng.randrange(0, 4)], "none": [],
              "one unstamped": [None], "one stamped": [1]}
    cases = [(v, d, c, r, a) for v in shapes.values() for d in (0, 1) for c in (0, 1) for r in (0, 1) for a in (0, 1)]
    check_replay(rule_exe, cases)
    assert classes([0, 1, 0, 0, 1, 0], True) == [REST, STAMPED, CARRIED, CARRIED, STAMPED, CARRIED] and classes([0, 1, 0], False) == [REST, STAMPED, REST]
    # by hand: a record leaves intact and in order, in both directions; the leading lines are the rest
    values = [None, 9, None, None, 2, None, 9, None]
    up, down, dropped = replay(rule_exe, [(values, 0, 1, 1, 0), (values, 1, 1, 1, 0), (values, 1, 0, 0, 0)])
    assert up["index"] == [4, 5, 1, 2, 3, 6, 7, 0] and up["values"] == [2, 2, 9, 9, 9, 9, 9, 0] and up["classes"] == [0, 1, 0, 1, 1, 0, 1, 2]
    assert down["index"] == [1, 2, 3, 6, 7, 4, 5, 0] and down["classes"] == [0, 1, 1, 0, 1, 0, 1, 2] and (down["m"], down["carried"], down["rest"]) == (7, 4, 1)
    assert dropped["index"] == [1, 6, 4] and (dropped["m"], dropped["carried"], dropped["rest"]) == (3, 0, 5)


def test_the_numpy_restatement_of_the_large_case_equals_the_oracle_on_every_draw():
    for seed, (n, share) in enumerate([(0, 0.5), (1, 0.0), (1, 1.0), (50, 0.3), (64, 0.9), (200, 0.05), (500, 0.5), (300, 1.0), (300, 0.0)]):
        rng = np.random.default_rng(seed)
        numbers = rng.integers(-40, 40, n) if seed % 2 else rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        stamped = rng.random(n) < share
        values = [int(v) if s else None for v, s in zip(numbers, stamped)]
        for d in (False, True):
            for c in (False, True):
                for r in (False, True):
                    index, out_values, out_class, _, _ = order_of(values, c, d, r)
                    g_index, g_values, g_class = np_sort(numbers, stamped, c, d, r)
                    assert g_index.tolist() == index and g_values.tolist() == out_values and g_class.tolist() == out_class, (n, share, d, c, r)
    assert CARRIED == 1 and STAMPED == 0
