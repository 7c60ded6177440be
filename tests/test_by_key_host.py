"""gx_lines_by_key / gx_text_lines_by_key as far as they go without a GPU: the symbols and struct layouts, every refusal that needs no
device -- gx_group_lines' and the call's own -- and "no device is an error, never a CPU path" behind them, the Python wrappers, and the
rule itself -- gorp_amd/csrc/gx_by_key.hpp, plain C++ -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into
tests/cpp/by_key_test.cpp and run as a program of its own: the keep rule, the digit plan, the sort and the bounds, against sorted()
(tests/by_key_oracle.py).  The numpy restatement the large GPU case is compared with equals the oracle on every small draw."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from by_key_oracle import draw, kept, np_by_key, passes, regroup
from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from group_oracle import NONE, group_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_lines_by_key", "gx_text_lines_by_key"]


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
    a = L.gx_lines_by_key.argtypes
    assert len(a) == 17 and a[6] == C.POINTER(N.gx_group_part) and a[8] == C.POINTER(N.gx_where_term) and a[10] is C.c_uint64 and a[11] is C.c_uint64
    assert a[12] is C.c_uint32 and a[13] == C.POINTER(N.gx_group_out) and a[14] == C.POINTER(N.gx_by_key_out) and a[15] == C.POINTER(N.gx_by_key_totals)
    assert a[16] == C.POINTER(N.gx_batch_opts)
    t = L.gx_text_lines_by_key.argtypes
    assert len(t) == 21 and t[3] == C.POINTER(N.gx_group_part) and t[7] is C.c_uint64 and t[10] == C.POINTER(N.gx_group_out) and t[17] == C.POINTER(N.gx_by_key_totals)
    # the layouts of include/gorp_hip.h: nine 8-byte fields; gx_group_totals' six words and three more
    assert C.sizeof(N.gx_by_key_out) == 72 and [(f[0], getattr(N.gx_by_key_out, f[0]).offset) for f in N.gx_by_key_out._fields_] == [
        ("out_index", 0), ("out_bytes", 8), ("out_offsets", 16), ("out_ids", 24), ("out_caps", 32), ("cap_lines", 40), ("out_bytes_cap", 48),
        ("key_out_lines", 56), ("key_out_units", 64)]
    assert C.sizeof(N.gx_by_key_totals) == 72 and C.sizeof(N.gx_group_totals) == 48
    assert [(f[0], getattr(N.gx_by_key_totals, f[0]).offset) for f in N.gx_by_key_totals._fields_] == [
        ("group", 0), ("keys_kept", 48), ("lines_out", 56), ("units_out", 64)]
    assert N.GX_BY_KEY_ALL_DIGITS == 2 and N.GX_GROUP_WEAK_HASH == 1
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["#define GX_BY_KEY_ALL_DIGITS 2u", "typedef struct gx_by_key_out {", "typedef struct gx_by_key_totals {", "uint64_t  cap_lines, out_bytes_cap;",
                       "uint64_t keys_kept, lines_out, units_out;", "computeIfAbsent(r.asMap().get(\"requestId\")", "README.md:26,63-79",
                       "max(min_lines, 1) <= key_lines[j]", "(key number, input line number)", "key_out_lines[n_keys] == lines_out", "terminator included",
                       "ONE host wait before any output", "33 bytes per INPUT line", "may now lie in the middle", "an output overlapping an input",
                       "out_caps on compact rows", "max_lines != 0 && min_lines > max_lines"]:
        assert text in header, text
    mirror = open(os.path.join(ROOT, "include", "gorp.hpp")).read()
    assert "linesByKey(" in mirror and "textLinesByKey(" in mirror
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_by_key.hpp")).read()
    assert "hip_runtime" not in rule and "gq_key_bits" in rule and "gq_lower_bound" in rule and "uint32_t gq_key_bits" not in rule   # reused, not copied


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    p = N.gx_group_part()
    p.extraction, p.key_group, p.value_group, p.reserved = extraction, key_group, value_group, reserved
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
    totals = N.gx_by_key_totals()
    room = (N.gx_measure_stats * 8)()
    o_index, o_bytes, o_off, o_ids, o_caps = np.zeros(8, np.uint32), np.zeros(64, np.uint8), np.zeros(9, np.uint32), np.zeros(64, np.int32), np.zeros((8, 6), np.int32)
    kol, kou = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    some_keys = N.gx_group_out()
    some_keys.max_keys = 4

    def full_out(**kw):
        b = N.gx_by_key_out(o_index.ctypes.data, o_bytes.ctypes.data, o_off.ctypes.data, o_ids.ctypes.data, o_caps.ctypes.data, 8, 64, kol.ctypes.data, kou.ctypes.data)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def both(parts, n_parts=None, terms=(), n_terms=None, min_lines=1, max_lines=0, caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals), n=3, off=offsets, flags=0,
             keys=some_keys, out=None, ids_arr=ids, **kw):
        arr = None
        if parts is not None:
            arr = (N.gx_group_part * max(1, len(parts)))()
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
        keys_ptr = None if keys is None else C.byref(keys)
        b = out if out is not None else N.gx_by_key_out()
        rc1 = L.gx_lines_by_key(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids_arr.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, min_lines, max_lines, flags,
                                keys_ptr, None if out is None else C.byref(b), totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_lines_by_key(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, min_lines, max_lines, flags, keys_ptr, b.out_bytes,
                                     b.out_bytes_cap, b.out_offsets, b.out_index, b.key_out_lines, b.key_out_units, totals_ptr, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    with_stats = N.gx_group_out()
    with_stats.key_stats = C.addressof(room)
    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None),       # totals == NULL
        dict(parts=None, n_parts=1),                                                  # gx_group_lines' refusals of the parts ...
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(extraction=2, key_group=3)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(2, 0, 3)]),
        dict(parts=[part(reserved=1)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        dict(parts=[part()], flags=4), dict(parts=[], flags=0x80000000), dict(parts=[part()], flags=2 | 8), dict(parts=[part()], flags=1 | 2 | 4),   # unknown flag bits
        dict(parts=[part()], keys=with_stats),                                        # key_stats without a value group
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),   # ... of the terms
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1),
        # the call's own: the bounds the wrong way round
        dict(parts=[part()], min_lines=2, max_lines=1), dict(parts=[], min_lines=2 ** 40, max_lines=7), dict(parts=[part()], min_lines=3, max_lines=2, out=full_out()),
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
                     (dict(parts=[part()], out=full_out(out_ids=ids.ctypes.data + 8)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_offsets=caps.ctypes.data + 4)), "overlaps"),
                     (dict(parts=[part()], out=full_out(key_out_units=ids.ctypes.data - 8)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_caps=offsets.ctypes.data - 16)), "overlaps"),
                     # a capacity that means "large enough" loses no refusal: no product of it wraps to nothing
                     (dict(parts=[part()], out=full_out(out_index=offsets.ctypes.data, cap_lines=2 ** 64 - 1)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_offsets=ids.ctypes.data - 4, cap_lines=2 ** 62)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_ids=caps.ctypes.data, cap_lines=2 ** 63)), "overlaps"),
                     (dict(parts=[part()], out=full_out(out_bytes=data.ctypes.data - 8, out_bytes_cap=2 ** 64 - 1)), "overlaps")):
        (rc, msg), _ = both(**kw)
        assert rc == N.GX_E_ARG and word in msg, (word, rc, msg)
    _, (rc, msg) = both(parts=[part()], out=full_out(out_bytes=text.ctypes.data + 8))
    assert rc == N.GX_E_ARG and "overlaps" in msg
    _, (rc, msg) = both(parts=[part()], out=full_out(key_out_lines=text.ctypes.data - 8))
    assert rc == N.GX_E_ARG and "overlaps" in msg
    limit = [
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
        dict(parts=[part()], keys=N.gx_group_out(None, 0, None, None, None, None, None, 2 ** 30 + 1)),   # max_keys above 2^30
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
            assert "no CPU fallback" not in msg
    # n of 2^32 - 1 and more; a line of 2^32 units or more, and offsets that go backwards (host offsets: read without a device)
    (rc, msg), _ = both(parts=[part()], n=0xFFFFFFFF)
    assert rc == N.GX_E_LIMIT and "2^32 - 1" in msg
    for off in (np.array([0, 2, 5, 5 + 2 ** 32], np.uint64), np.array([0, 2, 1, 7], np.uint64)):
        (rc, msg), _ = both(parts=[part()], off=off, offsets64=1)
        assert rc == N.GX_E_LIMIT and "4 G code units" in msg
    # parts or terms on dense ids without caps (the whole-file call makes its own)
    for kw in (dict(parts=[part()]), dict(parts=[], terms=[term()])):
        (rc, msg), (rc2, msg2) = both(caps_ptr=None, **kw)
        assert rc == N.GX_E_ARG and "caps" in msg
        assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part(0, 0, 0)]), dict(parts=[part()], keys=None), dict(parts=[part()], out=full_out()),
            dict(parts=[part()], min_lines=0), dict(parts=[part()], min_lines=5, max_lines=0), dict(parts=[part()], min_lines=1, max_lines=1),
            dict(parts=[part()], min_lines=2 ** 63, max_lines=2 ** 64 - 1), dict(parts=[part(0, 0, 0)], keys=with_stats),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BY_KEY_ALL_DIGITS),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH | N.GX_BY_KEY_ALL_DIGITS, out=full_out()),
            dict(parts=[part(2, 0), part()], terms=[term()] * 64), dict(parts=[part()], utf8=1),
            dict(parts=[part()], compact_results=2, ids_arr=np.zeros((3, 7), np.uint8)),
            dict(parts=[part()], compact_results=1, ids_arr=rows16, out=full_out(out_caps=None)),
            dict(parts=[part()], n=0xFFFFFFFE, device_pointers=1)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.lines_by_key(data, offsets, ids, caps, [("alpha", "x")], min_lines=2)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_lines_by_key(bytes(text), [("gamma", "z")], max_lines=1, where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.lines_by_key(data, offsets, ids, caps, [("alpha", "x")], min_lines=3, max_lines=2)
    assert ei.value.code == N.GX_E_ARG and "min_lines" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.lines_by_key(data, offsets, ids, None, [("alpha", "x")])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(ValueError):
        g.lines_by_key(data, offsets, ids, caps, [("alpha", "x")], utf8="units")
    with pytest.raises(ValueError):
        g.lines_by_key(data, offsets, ids, caps, [("alpha", "nope")])


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_by_key_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_lines_by_key(h, None, off, 1, id_ptr, None, None, 0, None, 0, 1, 0, 0, None, None, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    args = (None, 0, None, 0, 1, 0, 0, None, None, 0, None, None, None, None, C.byref(t), None, None, C.byref(o))
    assert L.gx_text_lines_by_key(None, None, 0, *args) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_lines_by_key(g._h.ptr, None, 5, *args) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("by_key") / "by_key_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "by_key_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def test_the_keep_rule_at_its_bounds(rule_exe):
    top = 2 ** 64 - 1
    cases = [(lines, lo, hi) for lines in (0, 1, 2, 3, 7, top) for lo in (0, 1, 2, 3, top) for hi in (0, 1, 2, 3, top)]
    # by hand: no key has no lines; min_lines 0 is min_lines 1; equal bounds keep exactly that count; max_lines 0 is no upper bound
    assert not kept(0, 0, None) and kept(1, 0, 0) and kept(1, 1, 1) and not kept(2, 1, 1) and kept(3, 3, 3) and not kept(2, 3, 3) and kept(10 ** 9, 2, 0)
    for (lines, lo, hi), line in zip(cases, run_cases(rule_exe, ["K %d %d %d" % c for c in cases])):
        assert int(line) == (1 if kept(lines, lo, hi) else 0), (lines, lo, hi)


def test_the_digit_plan(rule_exe):
    sizes = [0, 1, 2, 64, 65, 4096, 4097, 2 ** 18 + 1, 2 ** 24 + 1, 2 ** 30] + [2 ** b + d for b in (6, 12, 18, 24) for d in (-1, 0, 1)]
    cases = [(n, a) for n in sizes for a in (0, 1)]
    want_by_hand = {0: 0, 1: 0, 2: 1, 64: 1, 65: 2, 4096: 2, 4097: 3, 2 ** 18 + 1: 4, 2 ** 24 + 1: 5, 2 ** 30: 5}
    for (n, a), line in zip(cases, run_cases(rule_exe, ["P %d %d" % c for c in cases])):
        nums = [int(x) for x in line.split()]
        # ceil(log2(n_keys)) bits hold the key numbers 0 .. n_keys - 1
        bits = 0 if n <= 1 else (n - 1).bit_length()
        want = 5 if a else -(-bits // 6)
        assert want == passes(n, bool(a)) and (a or n not in want_by_hand or want == want_by_hand[n])
        assert nums[0] == want and nums[1] == want % 2 and nums[2:] == [6 * p for p in range(want)], (n, a, nums)


def test_the_sort_and_the_bounds_equal_sorted(rule_exe):
    rng = random.Random(11)
    cases = []
    for n_keys, m in ((1, 1), (1, 70), (2, 129), (64, 500), (65, 500), (4097, 3000), (2 ** 18 + 1, 2000), (2 ** 30, 300), (7, 0)):
        for all_digits in (0, 1):
            keys = [rng.randrange(n_keys) for _ in range(m)]
            if m > 2:
                keys[0], keys[-1] = n_keys - 1, 0
            cases.append((n_keys, all_digits, keys))
    cases.append((2, 0, [i & 1 for i in range(200)]))           # two keys strictly alternating
    cases.append((300, 0, list(range(299, -1, -1))))              # every entry its own key, descending
    rows = ["S %d %d %d %s" % (n_keys, a, len(keys), " ".join(map(str, keys))) for n_keys, a, keys in cases]
    for (n_keys, a, keys), line in zip(cases, run_cases(rule_exe, rows)):
        nums = [int(x) for x in line.split()]
        m = len(keys)
        assert nums[:m] == sorted(range(m), key=lambda i: (keys[i], i)), (n_keys, a)
        shown = min(n_keys, 5000)
        assert nums[m:m + shown + 1] == [sum(1 for k in keys if k < j) for j in range(shown + 1)], (n_keys, a)
        assert nums[-1] == m and len(nums) == m + shown + 1 + (1 if shown < n_keys else 0)


def test_the_numpy_restatement_of_the_large_case_equals_the_oracle_on_every_draw():
    for seed, (n_lines, n_names) in enumerate([(0, 1), (1, 1), (50, 1), (64, 64), (200, 65), (500, 40), (300, 300), (1000, 257), (40, 100)]):
        for lo, hi in ((1, None), (2, None), (1, 1), (3, 5), (10 ** 6, None)):
            names, lengths = draw(n_lines, n_names, seed)
            keys, first, count, line_key = group_values([None if v < 0 else int(v) for v in names])
            order, kol, kou = regroup(line_key, count, lengths, lo, hi)
            g_key, g_lines, g_order, g_kol, g_kou = np_by_key(names, lengths, lo, hi)
            what = (n_lines, n_names, lo, hi)
            assert g_key.tolist() == line_key and g_lines.tolist() == count, what
            assert g_order.tolist() == order and g_kol.tolist() == kol and g_kou.tolist() == kou, what
            assert all(j == NONE or kept(count[j], lo, hi) == (i in set(order)) for i, j in enumerate(line_key))
