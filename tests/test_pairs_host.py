"""gx_group_pairs / gx_text_group_pairs as far as they go without a GPU: the structs, the symbols and the header's text, every refusal
that needs no device (and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into parts and
second groups, and the rule itself -- the pair hash and the find-or-insert of gorp_amd/csrc/gx_pairs.hpp, plain C++, with the host
policy -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into tests/cpp/pairs_test.cpp and run as a
program of its own, against a Python dict and a Python restatement of the probing (tests/pairs_oracle.py).  The numpy restatement that
the large GPU case is compared with is compared with the oracle here, on small draws of the same generator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, GroupParts
from group_oracle import NONE, hash_units
from pairs_oracle import draw, group_pairs, named_batch, np_pairs, pair_hash, probe_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_pairs", "gx_text_group_pairs"]


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


# ---------------------------------------------------------------------------
# structs, symbols, the header's text
# ---------------------------------------------------------------------------
def test_struct_layouts_symbols_and_header_text():
    O, T = N.gx_pairs_out, N.gx_pairs_totals
    assert C.sizeof(O) == 72
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("pair_units", 0), ("pair_units_cap", 8), ("pair_offsets", 16), ("pair_key", 24),
                                                                    ("pair_first_line", 32), ("pair_lines", 40), ("key_pairs", 48), ("line_pair", 56), ("max_pairs", 64)]
    assert C.sizeof(T) == 88 and T.group.offset == 0 and C.sizeof(N.gx_group_totals) == 48
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_[1:]] == [("n_pairs", 48), ("pair_units", 56), ("paired", 64), ("unpaired", 72), ("pairs_exact", 80)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["typedef struct gx_pairs_out {", "typedef struct gx_pairs_totals {", "const int32_t* second_groups", "keyed == paired +\n * unpaired",
                       "NOT IN SCOPE: stats per pair, quantiles per pair, ranking pairs, more than two texts", "pairs_exact = 0 and n_pairs = slots + 1",
                       "every second group is -1"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_pairs.hpp")).read()
    for text in ["no flag, no fence, no lane that waits for\n// another lane", "Not in scope: stats per pair, quantiles per pair, ranking pairs, more than two texts",
                 "pair_hash(uint64_t second_hash, uint32_t key_slot, bool weak)", "struct PairsHead"]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    return N.gx_group_part(extraction, key_group, value_group, reserved)


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
    buf = np.zeros(64, np.uint64)

    def both(parts, seconds="all", n_parts=None, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, pairs=True, outputs=(), max_keys=8, max_pairs=8, n=3,
             **kw):
        arr = None if parts is None else (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        if seconds == "all":
            seconds = [0] * n_parts
        sec = None if seconds is None else (C.c_int32 * max(1, len(seconds)))(*seconds)
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        keys = N.gx_group_out()
        keys.max_keys = max_keys
        out = N.gx_pairs_out()
        out.max_pairs = max_pairs
        out.pair_units_cap = 64
        for name in outputs:
            setattr(out, name, buf.ctypes.data)
        tot = N.gx_pairs_totals()
        tp = C.byref(tot) if totals else None
        pp = C.byref(out) if pairs else None
        rc1 = L.gx_group_pairs(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, sec, tarr, len(terms), flags, C.byref(keys),
                               pp, tp, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_pairs(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, sec, tarr, len(terms), flags, C.byref(keys), pp, tp, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    every_output = ("pair_units", "pair_offsets", "pair_key", "pair_first_line", "pair_lines", "key_pairs", "line_pair")
    arg = [
        # what gx_group_pairs adds
        dict(parts=[part()], seconds=None),                                         # second_groups == NULL with n_parts > 0
        dict(parts=[part()], seconds=None, pairs=False),
        dict(parts=[part()], seconds=[1]), dict(parts=[part()], seconds=[-2]),       # alpha has one group
        dict(parts=[part(extraction=2)], seconds=[3]), dict(parts=[part(), part(extraction=2)], seconds=[0, 3]),
        dict(parts=[part()], seconds=[1], pairs=False),                              # (checked whether or not pairs are asked for)
    ] + [dict(parts=[part(), part(extraction=2)], seconds=[-1, -1], outputs=(name,)) for name in every_output] + [
        # gx_group_lines' own
        dict(parts=None, n_parts=1),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(key_group=1)]), dict(parts=[part(extraction=1)], seconds=[-1]),
        dict(parts=[part(), part()], seconds=[0, 0]), dict(parts=[part(reserved=1)]),
        dict(parts=[part()], flags=2), dict(parts=[], flags=0x80000000),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()], max_pairs=2 ** 30 + 1), dict(parts=[], max_pairs=2 ** 40), dict(parts=[part()], seconds=[-1], max_pairs=2 ** 30 + 1),
        dict(parts=[part()], max_keys=2 ** 30 + 1), dict(parts=[part()] * 65, seconds=[0] * 65),
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[], outputs=every_output), dict(parts=[part()]), dict(parts=[part()], outputs=every_output),
            dict(parts=[part()], pairs=False), dict(parts=[part()], seconds=[-1]), dict(parts=[part()], seconds=[-1], pairs=False),
            dict(parts=[part(), part(extraction=2, key_group=1)], seconds=[-1, 2], outputs=every_output),
            dict(parts=[part(extraction=2, key_group=2, value_group=0)], seconds=[2]),                      # the key group itself is a second like any other
            dict(parts=[part()], max_pairs=0), dict(parts=[part()], max_pairs=2 ** 30), dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_pairs(data, offsets, ids, caps, [("gamma", "z", 0)])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_pairs(bytes(text), [("alpha", "x", "x")], where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.group_pairs(data, offsets, ids, caps, [("alpha", "x", None)])
    assert ei.value.code == N.GX_E_ARG and "every part's second group is -1" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.group_pairs(data, offsets, ids, caps, [("alpha", "x", "x")], max_pairs=2 ** 30 + 1)
    assert ei.value.code == N.GX_E_LIMIT


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_pairs_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_pairs(h, None, off, 1, id_ptr, None, None, 0, None, None, 0, 0, None, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_pairs(None, None, 0, None, 0, None, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_group_pairs(g._h.ptr, None, 5, None, 0, None, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_pair_parts_resolve_names_and_groups():
    g = three_rules()
    p, s = g.pair_parts([("alpha", "x", "x"), (2, "z", 0, 1)])
    assert isinstance(p, GroupParts) and p.n == 2 and p.has_values
    assert [(t.extraction, t.key_group, t.value_group) for t in list(p.array)[:p.n]] == [(0, 0, -1), (2, 2, 1)] and list(s)[:2] == [0, 0]
    assert g.pair_parts((p, s)) == (p, s)
    p, s = g.pair_parts([("gamma", 1, None), ("alpha", 0, 0)])
    assert list(s)[:2] == [-1, 0] and not p.has_values
    assert g.pair_parts([])[0].n == 0
    for spec in ([("alpha", "x")], [("alpha", "x", "x", None, 1)], [("alpha", "x", "y")], [("alpha", "x", 1)], [("gamma", "z", "y")], [("delta", "x", "x")],
                 [("alpha", "x", "x"), ("alpha", "x", None)]):
        with pytest.raises(ValueError):
            g.pair_parts(spec)


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairs") / "pairs_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pairs_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def hexed(units, wide=False):
    return "".join(("%04x" if wide else "%02x") % u for u in units) or "-"


def row_of(kind, items, weak, wide, slots=None):
    head = "%s %s %d " % (kind, "w" if wide else "b", 1 if weak else 0) + ("" if slots is None else "%d " % slots)
    return head + "%d %s" % (len(items), " ".join("%d:%s" % (k, hexed(v, wide)) for k, v in items))


def check_tables(exe, cases):
    """cases: (items, slots, weak, wide), items (key slot, second units).  The program's slots, loads and table against the restatement's,
    and the numbering the slots give against a Python dict's."""
    got = run_cases(exe, [row_of("T", items, weak, wide, slots) for items, slots, weak, wide in cases])
    parsed = []
    for (items, slots, weak, wide), row in zip(cases, got):
        left, right = row.split("|")
        found = [(None if s == "full" else int(s), int(loads)) for s, loads in (e.split("@") for e in left.split())]
        table = {int(s): (int(ln), int(tag)) for s, ln, tag in (e.split(":") for e in right.split())}
        want, want_table = probe_pairs(items, slots, weak)
        assert found == want and table == want_table, (items, slots, weak)
        if all(s is not None for s, _ in found):
            number, by_dict = {}, {}
            for (s, _), (k, v) in zip(found, items):
                number.setdefault(s, len(number))
                by_dict.setdefault((k, tuple(v)), len(by_dict))
                assert number[s] == by_dict[k, tuple(v)]
            assert len(number) == len(by_dict)
        parsed.append((found, table))
    return parsed


def test_sizes_and_hash_restated(pairs_exe):
    assert run_cases(pairs_exe, ["Z"]) == ["272 64 %d" % 2 ** 30]
    items = [(0, ()), (1, ()), (0, tuple(b"a")), (1, tuple(b"a")), (0xFFFFFFFE, tuple(b"a")), (7, tuple(range(1, 256))), (2 ** 31 - 1, (0,)), (3, (0, 0))]
    for weak in (False, True):
        got = [int(x) for x in run_cases(pairs_exe, [row_of("H", items, weak, False)])[0].split()]
        assert got == [pair_hash(v, k, weak) for k, v in items]
        assert len(set(got)) == len(items) or weak
        assert not weak or set(got) <= set(range(8))
    wide = [(5, (0x416, 0xFF11)), (5, (0x16,)), (6, (0x16,))]
    assert [int(x) for x in run_cases(pairs_exe, [row_of("H", wide, False, True)])[0].split()] == [pair_hash(v, k) for k, v in wide]
    # tag and first slot depend on BOTH: the same second under 64 key slots, and 64 seconds under one key slot, spread over tags and slots
    for many in ([pair_hash(tuple(b"path"), k) for k in range(64)], [pair_hash((q,), 9) for q in range(64)]):
        assert len({h >> 32 for h in many}) == 64 and len({h & 1023 for h in many}) > 48


def test_identity_cases(pairs_exe):
    ab_c = [(0, tuple(b"c")), (1, tuple(b"bc"))]          # ("ab","c") against ("a","bc"): keys ab and a hold slots 0 and 1
    swapped = [(0, tuple(b"b")), (1, tuple(b"a"))]        # ("a","b") against ("b","a")
    two_keys = [(0, tuple(b"s")), (1, tuple(b"s")), (0, tuple(b"s"))]
    empties = [(0, ()), (1, ()), (0, ()), (0, (0,))]
    for weak in (False, True):
        got = check_tables(pairs_exe, [(ab_c, 64, weak, False), (swapped, 64, weak, False), (two_keys, 64, weak, False), (empties, 64, weak, False)])
        slots = [[s for s, _ in found] for found, _ in got]
        assert slots[0][0] != slots[0][1] and slots[1][0] != slots[1][1]
        assert slots[2][0] == slots[2][2] != slots[2][1]
        assert slots[3][0] == slots[3][2] and len(set(slots[3])) == 3


def seeded_items(seed, count, n_key_slots, n_seconds, wide=False):
    rng = np.random.default_rng(seed)
    top = 0x10000 if wide else 256
    seconds = [tuple(int(x) for x in rng.integers(0, top, int(rng.integers(0, 7)))) for _ in range(n_seconds)]
    return [(int(rng.integers(0, n_key_slots)), seconds[int(rng.integers(0, n_seconds))]) for _ in range(count)]


def test_seeded_draws_strong_and_weak(pairs_exe):
    cases = []
    for seed in range(6):
        items = seeded_items(seed, 400, 1 + seed * 3, 5 + seed * 7, wide=seed % 2 == 1)
        distinct = len({(k, v) for k, v in items})
        slots = 64
        while slots < 2 * distinct:
            slots *= 2
        for weak in (False, True):
            cases.append((items, slots, weak, seed % 2 == 1))
    got = check_tables(pairs_exe, cases)
    assert all(s is not None for found, _ in got for s, _ in found)
    assert all(tag == 0 for (_, _, weak, _), (_, table) in zip(cases, got) if weak for _, tag in table.values())


def test_a_table_filled_to_its_last_slot_reports_full_after_exactly_n_slots_probes(pairs_exe):
    for weak in (False, True):
        pairs = sorted({(k, v) for k, v in seeded_items(11, 3000, 9, 40)})[:65]
        assert len(pairs) == 65
        full = pairs[:64]
        got = check_tables(pairs_exe, [(full, 64, weak, False), (full + full, 64, weak, False), (full + [pairs[64]] + full, 64, weak, False)])
        (f0, t0), (f1, t1), (f2, t2) = got
        assert all(s is not None for s, _ in f0 + f1) and len(t0) == 64
        assert f2[64] == (None, 64)                                               # GROUP_NONE after exactly n_slots loaded words
        assert [s for s, _ in f2[65:]] == [s for s, _ in f0] and t0 == t1 == t2   # the 65th left the table as it was
        assert NONE == 0xFFFFFFFF


def test_a_prefix_of_its_neighbour_is_another_pair(pairs_exe):
    long = tuple(b"q" * 299 + b"r")
    items = [(4, tuple(b"abc")), (4, tuple(b"ab")), (4, tuple(b"abcd")), (4, ()), (4, tuple(b"abd")), (4, tuple(b"abc")), (4, long), (4, long[:-1]), (5, long), (4, long)]
    for weak in (False, True):
        found, _ = check_tables(pairs_exe, [(items, 64, weak, False)])[0]
        slots = [s for s, _ in found]
        assert len(set(slots)) == 8 and slots[0] == slots[5] and slots[6] == slots[9] != slots[8]
    assert hash_units(()) != 0


# ---------------------------------------------------------------------------
# the numpy restatement of the large GPU case against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(0, 1, 1), (1, 1, 1), (300, 7, 5), (2000, 40, 9), (2000, 3, 200), (500, 400, 1)])
def test_the_numpy_restatement_equals_the_oracle_on_small_draws(shape):
    n, n_keys, n_seconds = shape
    kn, sn, extra = draw(n, n_keys, n_seconds, seed=n + n_keys)
    data, offsets, ids, caps = named_batch(kn, sn, extra)
    want = group_pairs(data, offsets, ids, caps, [(0, 0, -1)], [1], [], 1)
    line_key, key_lines, line_pair, pair_key, pair_first, pair_lines, key_pairs = np_pairs(kn, sn, n_seconds)
    assert line_key.tolist() == want["line_key"] and key_lines.tolist() == want["lines"] and line_pair.tolist() == want["line_pair"]
    assert pair_key.tolist() == [j for j, _ in want["pairs"]] and pair_first.tolist() == want["pair_first_line"] and pair_lines.tolist() == want["pair_lines"]
    assert key_pairs.tolist() == want["key_pairs"]
    assert [v for _, v in want["pairs"]] == [(int(sn[i]) & 255,) for i in want["pair_first_line"]]
    assert want["totals"]["unpaired"] == int(((kn >= 0) & (sn < 0)).sum())
