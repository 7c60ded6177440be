"""gx_group_quantiles / gx_text_group_quantiles as far as they go without a GPU: the symbols, every refusal that needs no device --
gx_group_lines' and gx_capture_quantiles' joined -- and "no device is an error, never a CPU path" behind them, the Python wrappers,
and the rule itself -- gorp_amd/csrc/gx_group_quantile.hpp, plain C++ -- built with g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined into tests/cpp/group_quantile_test.cpp and run as a program of its own: the digit plan, a host LSD sort
driven by it and the pick, against sorted() per key (tests/group_quantile_oracle.py)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from group_quantile_oracle import key_bits, plan_of
from quantile_oracle import ASKS, D32, INT64_MAX, INT64_MIN, parting_values, quantiles_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_quantiles", "gx_text_group_quantiles"]


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


def test_symbols_argtypes_and_header_text():
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    a = L.gx_group_quantiles.argtypes
    assert len(a) == 17 and a[6] == C.POINTER(N.gx_group_part) and a[10] == C.POINTER(N.gx_quantile) and a[13] == C.POINTER(N.gx_group_out)
    assert a[14] is C.c_void_p and a[15] == C.POINTER(N.gx_group_totals) and a[16] == C.POINTER(N.gx_batch_opts)
    t = L.gx_text_group_quantiles.argtypes
    assert len(t) == 16 and t[3] == C.POINTER(N.gx_group_part) and t[7] == C.POINTER(N.gx_quantile) and t[10] == C.POINTER(N.gx_group_out) and t[11] is C.c_void_p
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["gx_quantile_out* key_quantiles", "out->max_keys x n_quantiles rows"]:
        assert text in header
    mirror = open(os.path.join(ROOT, "include", "gorp.hpp")).read()
    assert "groupQuantiles(" in mirror and "textGroupQuantiles(" in mirror


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    p = N.gx_group_part()
    p.extraction, p.key_group, p.value_group, p.reserved = extraction, key_group, value_group, reserved
    return p


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


HALF = [(1, 2)]


def test_every_refusal_comes_before_the_look_at_the_device():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    totals = N.gx_group_totals()
    rows = (N.gx_quantile_out * 64)()
    some_out = N.gx_group_out()
    some_out.max_keys = 4

    def both(parts, n_parts=None, terms=(), n_terms=None, qs=HALF, n_qs=None, rows_ptr=C.addressof(rows), caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals),
             n=3, off=offsets, flags=0, out=some_out, **kw):
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
        qarr = None
        if qs is not None:
            qarr = (N.gx_quantile * max(1, len(qs)))()
            for i, (num, den) in enumerate(qs):
                qarr[i].num, qarr[i].den = num, den
        n_qs = len(qs) if n_qs is None else n_qs
        o = opts(**kw)
        out_ptr = None if out is None else C.byref(out)
        rc1 = L.gx_group_quantiles(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, qarr, n_qs, flags, out_ptr,
                                   rows_ptr, totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_quantiles(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, qarr, n_qs, flags, out_ptr, rows_ptr, totals_ptr, None, None,
                                        C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    with_stats = N.gx_group_out()
    with_stats.key_stats = C.addressof(rows)
    big = N.gx_group_out()
    big.max_keys = 2 ** 30 + 1
    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None),       # gx_group_lines': totals == NULL
        dict(parts=None, n_parts=1),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(extraction=2, key_group=3)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(2, 0, 3)]),
        dict(parts=[part(reserved=1)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        dict(parts=[part()], flags=2), dict(parts=[], flags=0x80000000),              # unknown flag bits
        dict(parts=[part()], out=with_stats),                                         # key_stats without a value_group
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1), dict(parts=[part()], qs=[], no_sync=1),
        # gx_capture_quantiles': quantiles == NULL with n_quantiles > 0, den == 0, num > den
        dict(parts=[part()], qs=None, n_qs=1), dict(parts=[], qs=None, n_qs=16), dict(parts=[part(0, 0, 0)], qs=None, n_qs=1, rows_ptr=None),
        dict(parts=[part()], qs=[(0, 0)]), dict(parts=[part(0, 0, 0)], qs=[(1, 2), (1, 0)]), dict(parts=[], qs=[(0, 0)]), dict(parts=[part()], qs=[(1, 0)], rows_ptr=None),
        dict(parts=[part()], qs=[(2, 1)]), dict(parts=[part(0, 0, 0)], qs=[(1, 1), (D32, D32 - 1)]), dict(parts=[], qs=[(3, 2)]), dict(parts=[], qs=[(3, 2)], out=None),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()], qs=ASKS + [(1, 2)]), dict(parts=[], qs=[(1, 2)] * 17), dict(parts=[part()], n_qs=0xFFFFFFFF),   # n_quantiles > GX_QUANTILE_MAX
        dict(parts=[part(0, 0, 0)], qs=[(1, 2)] * 17, rows_ptr=None),
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
        dict(parts=[part()], out=big),                                                # max_keys above 2^30
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
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part(0, 0, 0)]), dict(parts=[part()], qs=[]), dict(parts=[], qs=[]), dict(parts=[part(0, 0, 0)], qs=ASKS),
            dict(parts=[part()], qs=None, n_qs=0, rows_ptr=None), dict(parts=[part(0, 0, 0)], qs=[(0, 1), (1, 1), (0, D32), (D32, D32)]),
            dict(parts=[part(0, 0, 0)], rows_ptr=None),                               # key_quantiles == NULL with n_quantiles > 0 is legal
            dict(parts=[part(0, 0, 0)], out=None), dict(parts=[part(0, 0, 0)], out=None, rows_ptr=None),
            dict(parts=[part(2, 2, 0), part()], terms=[term(), term(extraction=2, group=1)]), dict(parts=[part(0, 0, 0)], flags=N.GX_GROUP_WEAK_HASH),
            dict(parts=[part(2, 0), part()], terms=[term()] * 64), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2),
            dict(parts=[part()], n=0xFFFFFFFE, device_pointers=1)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_quantiles(data, offsets, ids, caps, [("alpha", "x", "x")], [0.5])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_quantiles(bytes(text), [("gamma", "z", 0)], ["0.95", (1, 2)], where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.group_quantiles(data, offsets, ids, None, [("alpha", "x")], [0.5])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(GorpError) as ei:
        g.group_quantiles(data, offsets, ids, caps, [("alpha", "x")], [1.5])          # refused by quantile_asks, before the library
    assert ei.value.code == N.GX_E_ARG and "[0, 1]" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_quantiles(bytes(text), [("alpha", "x")], [0.5] * 17)
    assert ei.value.code == N.GX_E_LIMIT
    with pytest.raises(ValueError):
        g.group_quantiles(data, offsets, ids, caps, [("alpha", "x")], [0.5], utf8="units")
    with pytest.raises(ValueError):
        g.group_quantiles(data, offsets, ids, caps, [("alpha", "nope")], [0.5])


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_group_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_quantiles(h, None, off, 1, id_ptr, None, None, 0, None, 0, None, 0, 0, None, None, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_quantiles(None, None, 0, None, 0, None, 0, None, 0, 0, None, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_group_quantiles(g._h.ptr, None, 5, None, 0, None, 0, None, 0, 0, None, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_quantile") / "group_quantile_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "group_quantile_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def test_key_bits_and_the_number_of_key_digits(rule_exe):
    counts = [0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 2 ** 18, 2 ** 18 + 1, 2 ** 24 + 1, 2 ** 30, 2 ** 30 + 1, 2 ** 32 - 1]
    got = [int(x) for x in run_cases(rule_exe, ["B %d" % c for c in counts])]
    assert got == [key_bits(c) for c in counts]
    assert [-(-key_bits(c) // 6) for c in (1, 2, 64, 65, 4096, 4097)] == [0, 1, 1, 2, 2, 3]        # where the number of key digits changes


def rows_of(pairs, n_keys, asks):
    """the flat rows value rank below equal per (key, quantile) from sorted() per key; a key without numbers: zeros"""
    by_key = [[] for _ in range(n_keys)]
    for k, v in pairs:
        by_key[k].append(v)
    out = []
    for pop in by_key:
        s = sorted(pop)
        for r in quantiles_of(pop, asks):
            if pop:
                assert s[r["rank"] - 1] == r["value"] and s.count(r["value"]) == r["equal"] and sum(1 for x in s if x < r["value"]) == r["below"]
            out += [r["value"] or 0, r["rank"], r["below"], r["equal"]]
    return out


def check_sort(exe, cases, all_values=False):
    """cases: [(n_keys, pairs, asks)]"""
    lines = ["S %d %d %d %s %d %s" % (n_keys, 1 if all_values else 0, len(asks), " ".join("%d %d" % a for a in asks), len(pairs),
                                      " ".join("%d %d" % p for p in pairs)) for n_keys, pairs, asks in cases]
    for (n_keys, pairs, asks), g in zip(cases, run_cases(exe, lines)):
        nums = [int(x) for x in g.split()]
        mask, key_digits, buffer = plan_of([v for _, v in pairs], n_keys, all_values)
        # a digit is skipped exactly when no two candidates differ in it; the key digits below bits(n_keys - 1); the result's buffer
        assert nums[:3] == [mask, key_digits, buffer], (n_keys, pairs[:8], nums[:3], (mask, key_digits, buffer))
        assert nums[3] == 1, "the plan's passes do not leave the pairs ordered by (key number, value, input place)"
        assert nums[4:] == rows_of(pairs, n_keys, asks), (n_keys, pairs[:8], asks)


EDGE_ASKS = [(0, 1), (1, 1), (1, 2), (99, 100), (1, D32), (D32 - 1, D32)]            # ranks on a run's first and last element among them


def test_the_host_sort_by_the_digit_plan_and_the_pick_equal_sorted_per_key(rule_exe):
    rng = random.Random(11)
    cases = []
    # random populations: few and many keys, narrow and wide values, keys without numbers (n_keys above the numbers that appear)
    for _ in range(120):
        n_keys = rng.choice([1, 2, 3, 7, 64, 65, 300])
        span = rng.choice([0, 3, 300, 2 ** 20, 2 ** 62])
        m = rng.choice([0, 1, 2, 5, 64, 65, 700])
        used = rng.sample(range(n_keys), max(1, n_keys * 2 // 3))
        pairs = [(rng.choice(used), rng.randint(-span, span)) for _ in range(m)]
        asks = [rng.choice(EDGE_ASKS + [(rng.randint(0, 9), 9)]) for _ in range(rng.choice([1, 3, 16]))]
        cases.append((n_keys, pairs, asks))
    # values that differ in every 6-bit digit, and values that differ in none
    every = [sum(((j * 7 + d) % 64) << (6 * d) for d in range(11)) % 2 ** 64 - 2 ** 63 for j in range(64)]
    assert plan_of(every, 1)[0] == 2 ** 11 - 1
    cases.append((3, [(j % 3, v) for j, v in enumerate(every)], ASKS))
    cases.append((3, [(j % 3, 1234567) for j in range(100)], ASKS))
    assert plan_of([1234567] * 5, 3) == (0, 1, 1) and plan_of([5], 1) == (0, 0, 0)
    # one digit at a time: the top one (four bits: the sign among them), the bottom one, one in the middle
    for d in (10, 0, 5):
        vals = [((0x0123456789ABCDEF & ~(63 << (6 * d))) | (((x * 5) % 64) << (6 * d))) % 2 ** 64 - 2 ** 63 for x in range(64 if d < 10 else 16)]
        assert plan_of(vals, 1)[0] == 1 << d
        cases.append((2, [(j & 1, v) for j, v in enumerate(vals * 2)], EDGE_ASKS))
    # the ends of int64, negatives next to positives
    edge = [INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1, INT64_MAX - 1, -64, 63, -2 ** 32, 2 ** 32, INT64_MIN, INT64_MAX]
    cases.append((1, [(0, v) for v in edge], ASKS))
    cases.append((4, [(j % 4, v) for j, v in enumerate(edge * 3)], ASKS))
    cases.append((2, [(j & 1, v) for j, v in enumerate(parting_values() * 2)], ASKS))
    # 1, 2, 64, 65, 4 096 and 4 097 keys: the number of key digits changes; every key its own number, and every other key none
    for n_keys in (1, 2, 64, 65, 4096, 4097):
        cases.append((n_keys, [(n_keys - 1 - j, (j * 37) % 101 - 50) for j in range(n_keys)], [(1, 2), (0, 1)]))
        cases.append((n_keys, [(j, j % 5) for j in range(0, n_keys, 2)] + [(j, 7) for j in range(0, n_keys, 2)], [(1, 1), (1, 2)]))
    # no candidates at all
    cases.append((5, [], ASKS))
    cases.append((0, [], ASKS))
    check_sort(rule_exe, cases)
    # the measurement's other arm: every value digit sorted, the same rows
    check_sort(rule_exe, cases[:40] + cases[-16:], all_values=True)
