"""gx_group_lines / gx_text_group_lines as far as they go without a GPU: the structs and the symbols, every refusal that needs no device
(and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into parts, and the table itself --
the find-or-insert of gorp_amd/csrc/gx_group.hpp, plain C++, with the host policy -- built with g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined into tests/cpp/group_test.cpp and run as a program of its own, against a Python dict and a Python
restatement of the probing (tests/group_oracle.py)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, GroupParts
from group_oracle import NONE, group_values, hash_units, probe_table, slots_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_lines", "gx_text_group_lines"]


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
# structs, symbols, refusals
# ---------------------------------------------------------------------------
def test_struct_layouts_and_symbols():
    P, O, T = N.gx_group_part, N.gx_group_out, N.gx_group_totals
    assert C.sizeof(P) == 16
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("extraction", 0), ("key_group", 4), ("value_group", 8), ("reserved", 12)]
    assert C.sizeof(O) == 64
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("key_units", 0), ("key_units_cap", 8), ("key_offsets", 16), ("key_first_line", 24),
                                                                    ("key_lines", 32), ("key_stats", 40), ("line_key", 48), ("max_keys", 56)]
    assert C.sizeof(T) == 48
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("n_keys", 0), ("key_units", 8), ("lines", 16), ("keyed", 24), ("unset", 32), ("exact", 40)]
    assert N.GX_GROUP_WEAK_HASH == 1
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for name in NEW + ["typedef struct gx_group_part {", "typedef struct gx_group_out {", "typedef struct gx_group_totals {", "#define GX_GROUP_WEAK_HASH 1u"]:
        assert name in header


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
    stats = (N.gx_measure_stats * 8)()

    def both(parts, n_parts=None, terms=(), n_terms=None, caps_ptr=caps.ctypes.data, flags=0, totals=True, key_stats=False, max_keys=8, n=3, **kw):
        arr = None
        if parts is not None:
            arr = (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        tarr = None
        if terms is not None:
            tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        n_terms = len(terms) if n_terms is None else n_terms
        o = opts(**kw)
        out = N.gx_group_out()
        out.max_keys = max_keys
        if key_stats:
            out.key_stats = C.addressof(stats)
        tot = N.gx_group_totals()
        tp = C.byref(tot) if totals else None
        rc1 = L.gx_group_lines(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, tarr, n_terms, flags, C.byref(out), tp,
                               C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_lines(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, tarr, n_terms, flags, C.byref(out), tp, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        dict(parts=None, n_parts=1),                                          # parts == NULL with n_parts > 0
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),     # totals == NULL
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]),
        dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]), dict(parts=[part(extraction=1)]),   # beta has no group
        dict(parts=[part(extraction=2, key_group=3)]),
        dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(extraction=2, key_group=0, value_group=3)]),
        dict(parts=[part(), part(extraction=2), part()]),                     # two parts for one extraction
        dict(parts=[part(extraction=2, key_group=1), part(extraction=2, key_group=2)]),
        dict(parts=[part(reserved=1)]),
        dict(parts=[part()], flags=2), dict(parts=[], flags=0x80000000), dict(parts=[part()], flags=3),
        dict(parts=[part()], key_stats=True), dict(parts=[], key_stats=True),  # key_stats where no part has a value group
        # every refusal of a term
        dict(parts=[part()], terms=None, n_terms=1), dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], terms=[term(op=10)]), dict(parts=[part()], terms=[term(op=N.GX_WHERE_EQ, text_units=3)]),
        dict(parts=[], terms=[term(extraction=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[], utf8=2),
        dict(parts=[part()], no_sync=1, device_pointers=1), dict(parts=[], no_sync=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    limit = [
        dict(parts=[part()] * 65),
        dict(parts=[part()], terms=[term()] * 65),
        dict(parts=[part()], max_keys=2 ** 30 + 1), dict(parts=[], max_keys=2 ** 40),
    ]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    # 2^32 - 1 lines and more (nothing is read before the refusal; the whole-file call has its own limit, 4 GiB of text)
    for n in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
        (rc, msg), _ = both(parts=[part()], n=n)
        assert rc == N.GX_E_LIMIT, msg
    tot = N.gx_group_totals()
    assert L.gx_text_group_lines(g._h.ptr, text.ctypes.data, 2 ** 32, None, 0, None, 0, 0, None, C.byref(tot), None, None, None) == N.GX_E_LIMIT
    # a line of 2^32 code units and more, or offsets that go backwards: host offsets are looked at before the device is
    tot = N.gx_group_totals()
    arr = (N.gx_group_part * 1)(part())
    for off in (np.array([0, 2, 2 ** 32 + 3, 2 ** 32 + 3], np.uint64), np.array([0, 2, 1, 3], np.uint64), np.array([0, 2, 1, 3], np.uint32)):
        o = opts(offsets64=1 if off.dtype == np.uint64 else 0)
        assert L.gx_group_lines(g._h.ptr, data.ctypes.data, off.ctypes.data, 3, ids.ctypes.data, caps.ctypes.data, arr, 1, None, 0, 0, None, C.byref(tot),
                                C.byref(o)) == N.GX_E_LIMIT and "4 G" in N.last_error()
    o = opts(offsets64=1)
    assert L.gx_group_lines(g._h.ptr, data.ctypes.data, np.array([0, 2, 2 ** 32 + 1, 2 ** 32 + 3], np.uint64).ctypes.data, 3, ids.ctypes.data, caps.ctypes.data, arr, 1,
                            None, 0, 0, None, C.byref(tot), C.byref(o)) == N.GX_E_DEVICE                      # (2^32 - 1 units is a line like any other)
    # parts or terms on dense ids without caps (the whole-file call makes its own)
    for kw in (dict(parts=[part()]), dict(parts=[], terms=[term()])):
        (rc, msg), (rc2, msg2) = both(caps_ptr=None, **kw)
        assert rc == N.GX_E_ARG and "caps" in msg
        assert rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[part()]), dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], max_keys=0),
            dict(parts=[part()], max_keys=2 ** 30), dict(parts=[part(extraction=2, key_group=2, value_group=0)], key_stats=True),
            dict(parts=[part(extraction=2, key_group=1, value_group=1), part()], key_stats=True, terms=[term(), term(extraction=2, group=1)]),
            dict(parts=[part(extraction=2, key_group=0, value_group=2)]),                                   # (key_stats is optional)
            dict(parts=[part()], terms=[term()] * 64), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    (rc, msg), _ = both(parts=[part()], compact_results=3)
    assert rc == N.GX_E_ARG
    # 64 parts need 64 extractions
    wide = Gorp.construct([FlattenedExtraction("r%d" % k, [["text", "a"], ["extractor", "v", [["pattern", ".*"]]]]) for k in range(65)], host_only=True)
    tot = N.gx_group_totals()
    for count, want in ((64, N.GX_E_DEVICE), (65, N.GX_E_LIMIT)):
        arr = (N.gx_group_part * count)(*[part(extraction=k) for k in range(count)])
        assert L.gx_group_lines(wide._h.ptr, data.ctypes.data, offsets.ctypes.data, 3, ids.ctypes.data, caps.ctypes.data, arr, count, None, 0, 0, None, C.byref(tot),
                                None) == want
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_lines(data, offsets, ids, caps, [("alpha", "x")])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_lines(bytes(text), [("gamma", "z", 0)], where=[("gamma", "z", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.group_lines(data, offsets, ids, None, [("alpha", "x")])
    assert ei.value.code == N.GX_E_ARG
    with pytest.raises(GorpError) as ei:
        g.group_lines(data, offsets, ids, caps, [("alpha", "x")], max_keys=2 ** 30 + 1)
    assert ei.value.code == N.GX_E_LIMIT
    with pytest.raises(ValueError):
        g.group_lines(data, offsets, ids, caps, [("alpha", "x")], utf8="units")


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_group_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_lines(h, None, off, 1, id_ptr, None, None, 0, None, 0, 0, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_lines(None, None, 0, None, 0, None, 0, 0, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG and "bad argument" in N.last_error()
    assert L.gx_text_group_lines(g._h.ptr, None, 5, None, 0, None, 0, 0, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG and "bad argument" in N.last_error()


# ---------------------------------------------------------------------------
# Gorp.group_parts
# ---------------------------------------------------------------------------
def test_group_parts_resolve_names_and_groups():
    g = three_rules()
    p = g.group_parts([("alpha", "x"), (2, "z", 0)])
    assert isinstance(p, GroupParts) and p.n == 2 and p.has_values
    assert [(t.extraction, t.key_group, t.value_group, t.reserved) for t in list(p.array)[:p.n]] == [(0, 0, -1, 0), (2, 2, 0, 0)]
    assert g.group_parts(p) is p
    assert g.group_parts([]).n == 0 and not g.group_parts([]).has_values and not g.group_parts([("gamma", 1, None)]).has_values
    q = g.group_parts([("gamma", "z", "z"), (0, 0, "x")])
    assert [(t.extraction, t.key_group, t.value_group) for t in list(q.array)[:q.n]] == [(2, 2, 2), (0, 0, 0)]
    bad = [("delta", "x"), (3, 0), (-1, 0), ("alpha", "y"), ("alpha", 1), ("beta", 0),
           ("gamma", "y"),                      # two groups of gamma are called y
           ("gamma", "z", "y"), ("alpha", "x", "z"), ("alpha", "x", 1), ("alpha",), ("alpha", "x", None, 2)]
    for spec in bad:
        with pytest.raises(ValueError):
            g.group_parts([spec])
    with pytest.raises(ValueError):
        g.group_parts([("alpha", "x"), ("gamma", "z"), (0, 0)])       # two parts for one extraction
    with pytest.raises(ValueError):
        g.group_parts([("alpha", "x")] * 65)


# ---------------------------------------------------------------------------
# the table under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def group_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group") / "group_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "group_test.cpp"), "-o", exe]
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


def table_row(values, slots, weak=False, wide=False):
    return "T %s %d %d %d %s" % ("w" if wide else "b", 1 if weak else 0, slots, len(values), " ".join(hexed(v, wide) for v in values))


def check_tables(exe, cases):
    """cases: (values, slots, weak, wide).  The program's slots and table against the restatement's, and the dictionary encoding the
    slots give against a Python dict's."""
    got = run_cases(exe, [table_row(*c) for c in cases])
    for (values, slots, weak, wide), row in zip(cases, got):
        left, right = row.split("|")
        slot_of = [None if s == "full" else int(s) for s in left.split()]
        table = {int(s): (int(ln), int(tag)) for s, ln, tag in (e.split(":") for e in right.split())}
        want_slots, want_table = probe_table(values, slots, weak)
        assert slot_of == want_slots and table == want_table, (values, slots, weak)
        if None not in slot_of:
            keys, first, count, line_key = group_values([tuple(v) for v in values])
            number = {}
            for s in slot_of:
                number.setdefault(s, len(number))
            assert [number[s] for s in slot_of] == line_key and len(number) == len(keys)
            assert all(table[s][0] == first[j] for s, j in number.items())       # (one thread: the representative is the first line)
    return got


LONG = tuple(b"q" * 299 + b"r")
ALPHABET = [(), tuple(b"a"), tuple(b"b"), tuple(b"aa"), tuple(b"ab"), LONG]


def test_every_multiset_of_up_to_five_values(group_exe):
    cases = []
    for n in range(6):
        for combo in itertools.product(ALPHABET, repeat=n):
            cases.append((list(combo), 64, False, False))
    assert len(cases) == sum(6 ** n for n in range(6))
    check_tables(group_exe, cases)
    # ... and under the weak hash, where all values share eight hashes and tag 0
    weak = [(list(combo), 64, True, False) for n in (3, 5) for combo in itertools.product(ALPHABET, repeat=n)]
    got = check_tables(group_exe, weak)
    assert all(e.split(":")[2] == "0" for row in got for e in row.split("|")[1].split())
    assert {hash_units(v, True) for v in ALPHABET} <= set(range(8))


def test_hash_and_slots_restated(group_exe):
    values = ALPHABET + [tuple(range(1, 256)), (0,), (0, 0)]
    got = run_cases(group_exe, ["H b 0 %d %s" % (len(values), " ".join(hexed(v) for v in values)), "H b 1 %d %s" % (len(values), " ".join(hexed(v) for v in values)),
                                "H w 0 2 %s %s" % (hexed((0x416, 0xFF11), True), hexed((0x16,), True))])
    assert [int(x) for x in got[0].split()] == [hash_units(v) for v in values] and len(set(got[0].split())) == len(values)
    assert [int(x) for x in got[1].split()] == [hash_units(v, True) for v in values]
    assert [int(x) for x in got[2].split()] == [hash_units((0x416, 0xFF11)), hash_units((0x16,))]
    sizes = [0, 1, 32, 33, 64, 65, 1000, 2 ** 20, 2 ** 20 + 1, 2 ** 30]
    assert [int(x) for x in run_cases(group_exe, ["S %d" % m for m in sizes])] == [slots_for(m) for m in sizes] == [64, 64, 64, 128, 128, 256, 2048, 2 ** 21, 2 ** 22, 2 ** 31]


def distinct(count, seed, lengths=(1, 12)):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < count:
        out.add(tuple(int(x) for x in rng.integers(0, 256, int(rng.integers(lengths[0], lengths[1])))))
    return sorted(out)


def test_a_table_of_64_slots_takes_64_keys_and_reports_the_65th_as_full(group_exe):
    for weak in (False, True):
        keys = distinct(65, 3)
        full = keys[:64]
        rows = check_tables(group_exe, [(full, 64, weak, False), (full + full, 64, weak, False), (full + [keys[64]] + full, 64, weak, False)])
        assert "full" not in rows[0] and "full" not in rows[1] and rows[2].split().count("full") == 1
        # the 65th left the table as it was, and every key is still found behind it
        assert rows[0].split("|")[1] == rows[1].split("|")[1] == rows[2].split("|")[1] and len(rows[0].split("|")[1].split()) == 64
        assert rows[2].split("|")[0].split()[65:] == rows[0].split("|")[0].split()


def test_probing_wraps_from_the_last_slot_to_slot_0(group_exe):
    at_end = [v for v in distinct(4000, 5) if hash_units(v) & 63 in (62, 63)][:6]
    assert len(at_end) == 6
    values = at_end + at_end[::-1]
    row = check_tables(group_exe, [(values, 64, False, False)])[0]
    slots = [int(s) for s in row.split("|")[0].split()]
    assert {62, 63, 0, 1, 2} <= set(slots[:6]) and slots[6:] == slots[:6][::-1]


def test_a_prefix_of_its_neighbour_is_another_key(group_exe):
    # equal units, different lengths; values that differ in the last unit only; all under the weak hash too, where the tag says nothing
    values = [tuple(b"abc"), tuple(b"ab"), tuple(b"abcd"), tuple(b"a"), (), tuple(b"abd"), tuple(b"abc"), LONG, LONG[:-1], LONG[:-1] + (ord("s"),), LONG, ()]
    for weak in (False, True):
        row = check_tables(group_exe, [(values, 64, weak, False)])[0]
        slots = row.split("|")[0].split()
        assert len(set(slots)) == 9 and slots[0] == slots[6] and slots[7] == slots[10] and slots[4] == slots[11]


def test_16_bit_units(group_exe):
    values = [(0x31,), (0xFF11,), (0x31, 0xFF11), (0x3100,), (0x0031, 0x0000), (), (0xFF11,), (0x416, 0x16), (0x16, 0x416), (0x31,)]
    for weak in (False, True):
        row = check_tables(group_exe, [(values, 64, weak, True)])[0]
        slots = row.split("|")[0].split()
        assert len(set(slots)) == 8 and slots[1] == slots[6] and slots[0] == slots[9]
    assert hash_units((0x3100,)) != hash_units((0x00, 0x31)) and NONE == 0xFFFFFFFF
