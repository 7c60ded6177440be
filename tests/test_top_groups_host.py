"""gx_top_groups / gx_text_top_groups as far as they go without a GPU: the symbols and struct layouts, every refusal that needs no
device -- gx_group_lines' and the call's own -- and "no device is an error, never a CPU path" behind them, the Python wrappers, and the
rule itself -- gorp_amd/csrc/gx_top_groups.hpp, plain C++ -- built with g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined into tests/cpp/top_groups_test.cpp and run as a program of its own: the key map, the digit plan, the
select and `chosen`, against sorted() (tests/top_groups_oracle.py)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from top_groups_oracle import M64, TOP_GROUPS_MAX, plan_of, rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_top_groups", "gx_text_top_groups"]
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63


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
    a = L.gx_top_groups.argtypes
    assert len(a) == 17 and a[6] == C.POINTER(N.gx_group_part) and a[8] == C.POINTER(N.gx_where_term) and a[10] is C.c_uint32 and a[12] is C.c_uint64
    assert a[14] == C.POINTER(N.gx_top_groups_out) and a[15] == C.POINTER(N.gx_top_groups_totals) and a[16] == C.POINTER(N.gx_batch_opts)
    t = L.gx_text_top_groups.argtypes
    assert len(t) == 16 and t[3] == C.POINTER(N.gx_group_part) and t[9] is C.c_uint64 and t[11] == C.POINTER(N.gx_top_groups_out)
    # the layouts of include/gorp_hip.h: nine 8-byte fields; gx_group_totals' six words and six more
    assert C.sizeof(N.gx_top_groups_out) == 72 and [f[0] for f in N.gx_top_groups_out._fields_] == [
        "key_units", "key_units_cap", "key_offsets", "key_number", "key_first_line", "key_lines", "key_stats", "line_rank", "cap_keys"]
    assert N.gx_top_groups_out.cap_keys.offset == 64 and N.gx_top_groups_out.line_rank.offset == 56
    assert C.sizeof(N.gx_top_groups_totals) == 96 and C.sizeof(N.gx_group_totals) == 48
    assert [(f[0], getattr(N.gx_top_groups_totals, f[0]).offset) for f in N.gx_top_groups_totals._fields_] == [
        ("group", 0), ("candidates", 48), ("n_top", 56), ("units_top", 64), ("last_lo", 72), ("last_hi", 80), ("ties_left", 88)]
    assert (N.GX_RANK_LINES, N.GX_RANK_NUMBERS, N.GX_RANK_SUM, N.GX_RANK_MAX, N.GX_RANK_MIN) == (0, 1, 2, 3, 4)
    assert N.GX_TOP_GROUPS_SMALLEST == 2 and N.GX_TOP_GROUPS_MAX == TOP_GROUPS_MAX == 4096
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["enum { GX_RANK_LINES = 0, GX_RANK_NUMBERS, GX_RANK_SUM, GX_RANK_MAX, GX_RANK_MIN };", "#define GX_TOP_GROUPS_SMALLEST 2u",
                       "#define GX_TOP_GROUPS_MAX 4096u", "uint64_t last_lo; int64_t last_hi;", "uint64_t  cap_keys;"]:
        assert text in header, text
    mirror = open(os.path.join(ROOT, "include", "gorp.hpp")).read()
    assert "topGroups(" in mirror and "textTopGroups(" in mirror
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_top_groups.hpp")).read()
    assert "MEAN" in rule and "192-bit" in rule                                    # the header says what is left out, and why


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
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    totals = N.gx_top_groups_totals()
    room = (N.gx_measure_stats * 8)()
    some_out = N.gx_top_groups_out()
    some_out.cap_keys = 4

    def both(parts, n_parts=None, terms=(), n_terms=None, rank_by=N.GX_RANK_LINES, n_wanted=3, max_keys=4, caps_ptr=caps.ctypes.data, totals_ptr=C.byref(totals),
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
        o = opts(**kw)
        out_ptr = None if out is None else C.byref(out)
        rc1 = L.gx_top_groups(g._h.ptr, data.ctypes.data, off.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, rank_by, n_wanted, max_keys, flags,
                              out_ptr, totals_ptr, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_top_groups(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, rank_by, n_wanted, max_keys, flags, out_ptr, totals_ptr, None,
                                   None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    with_stats = N.gx_top_groups_out()
    with_stats.key_stats = C.addressof(room)
    arg = [
        dict(parts=[part()], totals_ptr=None), dict(parts=[], totals_ptr=None),       # totals == NULL
        dict(parts=None, n_parts=1),                                                  # gx_group_lines' refusals of the parts ...
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]), dict(parts=[part(extraction=1)]), dict(parts=[part(extraction=2, key_group=3)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(2, 0, 3)]),
        dict(parts=[part(reserved=1)]),
        dict(parts=[part(), part()]), dict(parts=[part(2, 1), part(), part(2, 0)]),   # two parts for one extraction
        dict(parts=[part()], flags=4), dict(parts=[], flags=0x80000000), dict(parts=[part()], flags=2 | 8),   # unknown flag bits
        dict(parts=[part()], out=with_stats),                                         # key_stats without a value group
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),   # ... of the terms
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1),
        # the call's own: rank_by out of range; a rank by numbers where no part has a value group
        dict(parts=[part()], rank_by=5), dict(parts=[part(0, 0, 0)], rank_by=0xFFFFFFFF), dict(parts=[], rank_by=5),
        dict(parts=[part()], rank_by=N.GX_RANK_NUMBERS), dict(parts=[part()], rank_by=N.GX_RANK_SUM), dict(parts=[part(), part(2, 0)], rank_by=N.GX_RANK_MAX),
        dict(parts=[], rank_by=N.GX_RANK_MIN), dict(parts=[part()], rank_by=N.GX_RANK_MIN, out=None),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()], n_wanted=N.GX_TOP_GROUPS_MAX + 1), dict(parts=[], n_wanted=0xFFFFFFFF), dict(parts=[part(0, 0, 0)], n_wanted=4097, out=None),
        dict(parts=[part()] * 65),                                                    # (before "two parts for one extraction")
        dict(parts=[part()], terms=[term()] * 65),
        dict(parts=[part()], max_keys=2 ** 30 + 1),                                   # max_keys above 2^30
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
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part(0, 0, 0)]), dict(parts=[part()], n_wanted=0), dict(parts=[], n_wanted=0),
            dict(parts=[part()], n_wanted=N.GX_TOP_GROUPS_MAX), dict(parts=[part(0, 0, 0)], out=None), dict(parts=[part(0, 0, 0)], out=with_stats),
            dict(parts=[part(0, 0, 0), part(2, 1)], rank_by=N.GX_RANK_MAX),           # one part with a value group beside one without
            dict(parts=[part(2, 2, 0), part()], terms=[term(), term(extraction=2, group=1)], rank_by=N.GX_RANK_SUM),
            dict(parts=[part(0, 0, 0)], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part(0, 0, 0)], flags=N.GX_TOP_GROUPS_SMALLEST, rank_by=N.GX_RANK_MIN),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH | N.GX_TOP_GROUPS_SMALLEST),
            dict(parts=[part(2, 0), part()], terms=[term()] * 64), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2),
            dict(parts=[part()], max_keys=0), dict(parts=[part()], max_keys=2 ** 30),
            dict(parts=[part()], n=0xFFFFFFFE, device_pointers=1)]
    for rank_by in range(5):
        fine.append(dict(parts=[part(0, 0, 0)], rank_by=rank_by))
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.top_groups(data, offsets, ids, caps, [("alpha", "x", "x")], 10, by="sum")
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_top_groups(bytes(text), [("gamma", "z", 0)], 3, by="max", largest=False, where=[("gamma", "z", "set")], line_rank=True)
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.top_groups(data, offsets, ids, None, [("alpha", "x")], 10)
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(GorpError) as ei:
        g.top_groups(data, offsets, ids, caps, [("alpha", "x")], 10, by="numbers")
    assert ei.value.code == N.GX_E_ARG and "value_group" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_top_groups(bytes(text), [("alpha", "x")], 4097)
    assert ei.value.code == N.GX_E_LIMIT
    with pytest.raises(ValueError):
        g.top_groups(data, offsets, ids, caps, [("alpha", "x")], 10, by="mean")
    with pytest.raises(ValueError):
        g.top_groups(data, offsets, ids, caps, [("alpha", "x")], 10, utf8="units")
    with pytest.raises(ValueError):
        g.top_groups(data, offsets, ids, caps, [("alpha", "nope")], 10)


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    t = N.gx_top_groups_totals()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_top_groups(h, None, off, 1, id_ptr, None, None, 0, None, 0, 0, 1, 0, 0, None, C.byref(t), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_top_groups(None, None, 0, None, 0, None, 0, 0, 1, 0, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()
    assert L.gx_text_top_groups(g._h.ptr, None, 5, None, 0, None, 0, 0, 1, 0, 0, None, C.byref(t), None, None, C.byref(o)) == N.GX_E_ARG
    assert "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_groups") / "top_groups_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "top_groups_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def words(v):
    """a signed 128-bit value as (int64 hi, uint64 lo)"""
    return v >> 64, v & M64


def check_select(exe, cases):
    """cases: [(values, n_wanted, smallest)]"""
    rows = ["S %d %d %d %s" % (1 if smallest else 0, n_wanted, len(values), " ".join("%d %d" % words(v) for v in values)) for values, n_wanted, smallest in cases]
    for (values, n_wanted, smallest), line in zip(cases, run_cases(exe, rows)):
        nums = [int(x) for x in line.split()]
        top, last, ties_left = rank(list(enumerate(values)), n_wanted, largest=not smallest)
        plan = plan_of(values, smallest)
        what = (values[:6], n_wanted, smallest)
        # a digit is selected on exactly when two candidates differ in it -- and only when something is wanted
        assert nums[0] == plan and nums[1] == (bin(plan).count("1") if top else 0), (what, nums[:2], plan)
        assert nums[2] == len(top) == min(n_wanted, len(values)), what
        assert nums[3:5] == list(words(last if top else 0)) and nums[5] == ties_left, (what, nums[3:6], last, ties_left)
        assert nums[6] == 1, "tg_value(tg_key(v)) != v, or the chosen are not n_top"
        assert nums[7:] == [j for j, _ in top], what


def test_the_key_map_the_digit_plan_the_select_and_chosen_equal_sorted(rule_exe):
    rng = random.Random(23)
    cases = []
    counts = lambda m: [0, 1, m, TOP_GROUPS_MAX]
    # random 128-bit rank values, narrow and wide, with repeats
    for _ in range(60):
        m = rng.choice([1, 2, 5, 64, 65, 300])
        span = rng.choice([0, 3, 300, 2 ** 40, 2 ** 70, 2 ** 127 - 1])
        values = [rng.randint(-span, span) for _ in range(m)]
        for n_wanted in counts(m) + [rng.randint(0, m + 2)]:
            cases.append((values, n_wanted, rng.random() < 0.5))
    # values that differ only in the high word, and only in the low word
    high = [(h << 64) + 12345 for h in (-3, 7, 0, -1, 7, 2 ** 62, -2 ** 63, 1)]
    low = [(5 << 64) + x for x in (0, M64, 1, 2 ** 63, 2 ** 63 - 1, 77, 77, 2 ** 32)]
    assert plan_of(high) & 0xFF == 0 and plan_of(high) >> 8 and plan_of(low) >> 8 == 0 and plan_of(low) & 0xFF
    # INT64_MIN / INT64_MAX as max and min (sign-extended), and the sums the issue names
    ends = [INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1, INT64_MAX - 1, INT64_MIN, INT64_MAX]
    sums = [-2 ** 64, 2 ** 64 - 2, 2 ** 65, 0, -1, 2 ** 64, -2 ** 64 - 1, 2 ** 65, 4 * INT64_MAX, 4 * INT64_MIN]
    every = [sum(((j * 7 + d * 3) % 256) << (8 * d) for d in range(16)) - 2 ** 127 for j in range(64)]      # the keys differ in all sixteen digits
    assert plan_of(every) == 0xFFFF and plan_of([42] * 9) == 0 and plan_of([]) == 0
    for values in (high, low, ends, sums, every, [42] * 9, [-7] * 300, []):
        for n_wanted in counts(len(values)) + [len(values) // 2, len(values) + 1]:
            for smallest in (False, True):
                cases.append((values, n_wanted, smallest))
    # one digit at a time: the top one (the sign among its bits), the bottom one, the two around the words' seam
    for d in (15, 0, 7, 8):
        values = [(((0x0123456789ABCDEF0123456789ABCDEF & ~(0xFF << (8 * d))) | (((x * 37) % 256) << (8 * d))) & (2 ** 128 - 1)) - 2 ** 127 for x in range(100)]
        assert plan_of(values) == 1 << d
        cases += [(values, 10, False), (values, 10, True), (values, 100, False)]
    check_select(rule_exe, cases)


def test_rank_values_from_a_slots_words(rule_exe):
    """tg_rank_value: which keys are candidates, and the 128-bit value of each kind; without values the stats words are never read"""
    # lines numbers min max, and the sum as (sum of low 32 bits, sum of floor(v / 2^32)) of the numbers listed
    def row(rank_by, has_values, lines, numbers_list):
        lo = sum(v & 0xFFFFFFFF for v in numbers_list)
        hi = sum(v >> 32 for v in numbers_list)
        mn, mx = (min(numbers_list), max(numbers_list)) if numbers_list else (INT64_MAX, INT64_MIN)
        return "V %d %d %d %d %d %d %d %d" % (rank_by, has_values, lines, len(numbers_list), mn, mx, lo & M64, hi)
    pops = [[], [5], [-5, -6], [INT64_MAX] * 4, [INT64_MIN] * 4, [INT64_MIN, INT64_MAX], [INT64_MAX, INT64_MAX, 2], [-1] * 3, [2 ** 32, -2 ** 32, 7]]
    rows, want = [], []
    for pop in pops:
        for rank_by, value in ((0, 9), (1, len(pop)), (2, sum(pop)), (3, max(pop) if pop else 0), (4, min(pop) if pop else 0)):
            rows.append(row(rank_by, 1, 9, pop))
            cand = rank_by <= 1 or len(pop) >= 1
            want.append("%d %d %d" % ((1,) + words(value) if cand else (0, 0, 0)))
    rows += [row(0, 0, 3, []), row(1, 0, 3, []), row(2, 0, 3, [])]
    want += ["1 0 3", "0 0 0", "0 0 0"]
    assert run_cases(rule_exe, rows) == want


def test_the_numpy_restatement_of_the_large_case_equals_the_oracle_on_every_draw():
    """tests/test_gpu_top_groups.py compares its large case with top_groups_oracle.np_top; here np_top is compared with the rule's own
    restatement (sorted() over Python ints) on smaller draws of the same generator.  No draw is left out: every line has a key and a
    number."""
    from top_groups_oracle import np_top, skewed_draw
    for seed in range(6):
        names, values = skewed_draw(3000, 900, seed)
        number, per_key = {}, []
        for name, v in zip(names.tolist(), values.tolist()):
            if name not in number:
                number[name] = len(per_key)
                per_key.append([])
            per_key[number[name]].append(v)
        for by, value in (("lines", len), ("numbers", len), ("sum", sum), ("max", max), ("min", min)):
            for largest in (True, False):
                for n_wanted in (0, 1, 10, 500, 4096):
                    cand = [(j, value(pop)) for j, pop in enumerate(per_key)]
                    top, last, ties_left = rank(cand, n_wanted, largest)
                    order, v, n_keys, ties = np_top(names, values, n_wanted, by, largest)
                    assert n_keys == len(per_key) and order.tolist() == [j for j, _ in top] and v.tolist() == [x for _, x in top] and ties == ties_left
