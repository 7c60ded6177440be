"""gx_bucket_lines / gx_text_bucket_lines as far as they go without a GPU: the structs, the symbols and the header's text, every refusal
that needs no device (and "no device is an error, never a CPU path" behind them), the Python side's resolution of names into parts, and
the rule itself -- bucket_of, the hash, the find-or-insert and the digit plan of gorp_amd/csrc/gx_bucket.hpp, plain C++, with the host
policy -- built with g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined into tests/cpp/bucket_test.cpp and run as a program
of its own, against Python's // on unbounded ints and a Python restatement of the probing (tests/bucket_oracle.py).  The numpy
restatement that the large GPU case is compared with is compared with the oracle here, on small draws of the same generator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import BucketParts, FlattenedExtraction, Gorp, GorpError
from bucket_oracle import (INT64_MAX, INT64_MIN, M64, NONE, bucket_hash, bucket_lines, bucket_of, digits_batch, digits_of, draw, np_buckets, probe_words,
                           word_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_bucket_lines", "gx_text_bucket_lines"]


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
    P, O, T = N.gx_bucket_part, N.gx_bucket_out, N.gx_bucket_totals
    assert C.sizeof(P) == 16 and [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("extraction", 0), ("number_group", 4), ("value_group", 8), ("reserved", 12)]
    assert C.sizeof(O) == 48
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("bucket_number", 0), ("bucket_first_line", 8), ("bucket_lines", 16), ("bucket_stats", 24),
                                                                    ("line_bucket", 32), ("max_buckets", 40)]
    assert C.sizeof(T) == 72
    assert [(f, getattr(T, f).offset) for f, _ in T._fields_] == [("n_buckets", 0), ("lines", 8), ("bucketed", 16), ("unset", 24), ("not_numbers", 32),
                                                                    ("out_of_range", 40), ("exact", 48), ("first_bucket", 56), ("last_bucket", 64)]
    assert N.GX_BUCKET_ALL_DIGITS == 2 and N.GX_GROUP_WEAK_HASH == 1
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    for text in NEW + ["typedef struct gx_bucket_part {", "typedef struct gx_bucket_out {", "typedef struct gx_bucket_totals {", "#define GX_BUCKET_ALL_DIGITS 2u",
                       "Math.floorDiv(Instant.parse(r.asMap().get(\"ts\")).toEpochMilli() - origin, 60_000L)", "perMinute.merge(b, 1L, Long::sum);",
                       "lines == bucketed + unset + not_numbers + out_of_range", "This differs from Java on purpose", "Math.subtractExact would throw",
                       "never origin + b * width", "exact = 0 and n_buckets = slots + 1", "an empty interval has no entry",
                       "NOT IN SCOPE: a text key beside the bucket (a series per verb), empty buckets filled in, calendar widths (months, local days),\n"
                       " * quantiles per bucket"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_bucket.hpp")).read()
    for text in ["no flag, no fence, no lane that waits for another lane", "This differs from Java on purpose", "Math.subtractExact would throw",
                 "Not in scope: a text key beside the bucket (a series per verb), empty buckets filled in, calendar widths (months, local days),\n"
                 "// quantiles per bucket", "bucket_of(int64_t v, int64_t origin, uint64_t width, int64_t* b)", "bucket_digits(uint64_t min_word, uint64_t max_word)",
                 "struct BucketHead", "why INT64_MIN is no bucket"]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule and "__int128" not in rule.split("#pragma once")[1]


def part(extraction=0, number_group=0, value_group=-1, reserved=0):
    return N.gx_bucket_part(extraction, number_group, value_group, reserved)


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

    def both(parts, n_parts=None, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, out=True, outputs=(), max_buckets=8, n=3, origin=0, width=1, **kw):
        arr = None if parts is None else (N.gx_bucket_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        bo = N.gx_bucket_out()
        bo.max_buckets = max_buckets
        for name in outputs:
            setattr(bo, name, buf.ctypes.data)
        tot = N.gx_bucket_totals()
        tp = C.byref(tot) if totals else None
        op = C.byref(bo) if out else None
        rc1 = L.gx_bucket_lines(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, origin, width, tarr, len(terms), flags, op,
                                tp, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_bucket_lines(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, origin, width, tarr, len(terms), flags, op, tp, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    every_output = ("bucket_number", "bucket_first_line", "bucket_lines", "line_bucket")
    arg = [
        # what gx_bucket_lines adds
        dict(parts=[part()], width=0), dict(parts=[part()], width=-1), dict(parts=[], width=0), dict(parts=[part()], width=INT64_MIN),
        dict(parts=[part()], outputs=("bucket_stats",)), dict(parts=[], outputs=("bucket_stats",)),
        dict(parts=[part()], flags=4), dict(parts=[part()], flags=8 | N.GX_BUCKET_ALL_DIGITS), dict(parts=[], flags=0x80000000),
        dict(parts=[part(reserved=1)]), dict(parts=[part(reserved=0x80000000)]),
        # gx_group_lines' own
        dict(parts=None, n_parts=1),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(number_group=1)]), dict(parts=[part(number_group=-1)]),
        dict(parts=[part(extraction=1)]), dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(extraction=2, value_group=3)]),
        dict(parts=[part(), part()]),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    (rc, msg), _ = both(parts=[part()], width=0)
    assert "width" in msg
    (rc, msg), _ = both(parts=[part()], outputs=("bucket_stats",))
    assert "bucket_stats without a value_group" in msg
    limit = [dict(parts=[part()], max_buckets=2 ** 30 + 1), dict(parts=[], max_buckets=2 ** 40), dict(parts=[part()] * 65)]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[], outputs=every_output), dict(parts=[part()]), dict(parts=[part()], outputs=every_output), dict(parts=[part()], out=False),
            dict(parts=[part(), part(extraction=2, number_group=1, value_group=0)], outputs=every_output + ("bucket_stats",)),
            dict(parts=[part(extraction=2, number_group=2, value_group=2)]),                               # the number group itself may be measured
            dict(parts=[part()], max_buckets=0), dict(parts=[part()], max_buckets=2 ** 30),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BUCKET_ALL_DIGITS | N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], width=INT64_MAX, origin=INT64_MIN), dict(parts=[part()], width=1, origin=INT64_MAX),
            dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.bucket_lines(data, offsets, ids, caps, [("gamma", "z", 0)], 60)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_bucket_lines(bytes(text), [("alpha", "x", "x")], 5, where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE
    with pytest.raises(GorpError) as ei:
        g.bucket_lines(data, offsets, ids, caps, [("alpha", "x")], 0)
    assert ei.value.code == N.GX_E_ARG and "width" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.bucket_lines(data, offsets, ids, caps, [("alpha", "x")], 1, max_buckets=2 ** 30 + 1)
    assert ei.value.code == N.GX_E_LIMIT


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_bucket_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_bucket_lines(h, None, off, 1, id_ptr, None, None, 0, 0, 1, None, 0, 0, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_bucket_lines(None, None, 0, None, 0, 0, 1, None, 0, 0, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_bucket_lines(g._h.ptr, None, 5, None, 0, 0, 1, None, 0, 0, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_bucket_parts_resolve_names_and_groups_and_a_text_origin():
    g = three_rules()
    p = g.bucket_parts([("alpha", "x", "x"), (2, "z", 0)])
    assert isinstance(p, BucketParts) and p.n == 2 and p.has_values
    assert [(t.extraction, t.number_group, t.value_group, t.reserved) for t in list(p.array)[:p.n]] == [(0, 0, 0, 0), (2, 2, 0, 0)]
    assert g.bucket_parts(p) is p
    p = g.bucket_parts([("gamma", 1), ("alpha", 0, None)])
    assert [(t.extraction, t.number_group, t.value_group) for t in list(p.array)[:p.n]] == [(2, 1, -1), (0, 0, -1)] and not p.has_values
    assert g.bucket_parts([]).n == 0
    for spec in ([("alpha",)], [("alpha", "x", "x", 1)], [("alpha", "x", "y")], [("alpha", "x", 1)], [("gamma", "y")], [("delta", "x")],
                 [("alpha", "x"), ("alpha", "x", None)], [("alpha", "x")] * 65):
        with pytest.raises(ValueError):
            g.bucket_parts(spec)
    # a text origin is read under the FIRST part's number format
    p = g.bucket_parts([("gamma", "z"), ("alpha", "x")])
    assert g._bucket_origin(p, 7) == 7 and g._bucket_origin(p, "-12") == -12 and g._bucket_origin(p, b"+3") == 3
    g.set_number_format("gamma", "z", "iso8601", 3)
    assert g._bucket_origin(p, "2026-01-03T00:00:00Z") == 1767398400000
    g.set_number_format("gamma", "z", "decimal", 2)
    assert g._bucket_origin(p, "1.5") == 150
    for bad in ("x", "", 2 ** 63, 1.5, True, None):
        with pytest.raises(ValueError):
            g._bucket_origin(p, bad)
    with pytest.raises(ValueError):
        g._bucket_origin(g.bucket_parts([]), "1")


# ---------------------------------------------------------------------------
# the rule under sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bucket_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bucket") / "bucket_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "bucket_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_cases(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    return out


def buckets_of(exe, triples):
    row = "B %d " % len(triples) + " ".join("%d %d %d" % t for t in triples)
    return [None if x == "x" else int(x) for x in run_cases(exe, [row])[0].split()]


CORNERS = [INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX]
WIDTHS = [1, 2, 3, 60_000, INT64_MAX]


def test_sizes(bucket_exe):
    assert run_cases(bucket_exe, ["Z"]) == ["672 64 %d 256 11" % 2 ** 30]


def test_bucket_of_on_the_corners(bucket_exe):
    triples = [(v, o, w) for v in CORNERS for o in CORNERS for w in WIDTHS]
    got = buckets_of(bucket_exe, triples)
    assert got == [bucket_of(*t) for t in triples]
    assert None in got and "touched" not in got
    # what the test itself relies on: the restatement is Python's floor division, limited to [INT64_MIN + 1, INT64_MAX]
    assert bucket_of(-1, 0, 60_000) == -1 and bucket_of(0, 0, 60_000) == 0 and bucket_of(-60_000, 0, 60_000) == -1 and bucket_of(-60_001, 0, 60_000) == -2
    assert bucket_of(INT64_MIN, 0, 1) is None and bucket_of(INT64_MIN + 1, 0, 1) == INT64_MIN + 1 and bucket_of(INT64_MAX, INT64_MIN, 1) is None
    assert bucket_of(INT64_MAX, INT64_MIN, 2) == INT64_MAX and bucket_of(INT64_MIN, INT64_MAX, 2) is None and bucket_of(INT64_MIN, INT64_MAX, 3) == -(2 ** 64 - 1) // 3


def test_bucket_of_on_exact_multiples_on_both_sides_of_the_origin(bucket_exe):
    triples = []
    for origin in (0, 7, -7, INT64_MAX - 10 ** 6, INT64_MIN + 10 ** 6):
        for width in (1, 2, 3, 60_000):
            for k in (-3, -2, -1, 0, 1, 2, 3):
                for d in (-1, 0, 1):
                    v = origin + k * width + d
                    if INT64_MIN <= v <= INT64_MAX:
                        triples.append((v, origin, width))
    got = buckets_of(bucket_exe, triples)
    assert got == [bucket_of(*t) for t in triples] and None not in got
    at = {t: b for t, b in zip(triples, got)}
    assert at[(7 - 60_000, 7, 60_000)] == -1 and at[(7 - 60_000 - 1, 7, 60_000)] == -2 and at[(7 - 1, 7, 60_000)] == -1 and at[(7, 7, 60_000)] == 0


def test_bucket_of_results_of_int64_min_and_beyond_are_out_of_range(bucket_exe):
    triples = [(INT64_MIN, 0, 1), (INT64_MIN, 1, 1), (INT64_MIN, INT64_MAX, 1), (INT64_MIN, INT64_MAX, 2), (-2, INT64_MAX, 1), (-1, INT64_MAX, 1),   # ... and below
               (INT64_MAX, -1, 1), (INT64_MAX, INT64_MIN, 1), (0, INT64_MIN, 1), (1, INT64_MIN + 1, 1),                                                  # ... and above
               (INT64_MIN + 1, 0, 1), (0, INT64_MAX, 1), (INT64_MIN, 0, 2), (INT64_MAX, 0, 1), (-1, INT64_MIN, 1), (INT64_MAX, INT64_MIN, 2)]            # the last ones inside
    got = buckets_of(bucket_exe, triples)
    assert got == [bucket_of(*t) for t in triples]
    assert got[:10] == [None] * 10 and got[10:] == [INT64_MIN + 1, -INT64_MAX, -2 ** 62, INT64_MAX, INT64_MAX, INT64_MAX]


def test_bucket_of_on_seeded_random_triples(bucket_exe):
    rng = np.random.default_rng(2026)
    triples = []
    for q in range(10_000):
        bits = int(rng.integers(1, 65))
        v, o = (int(x) - 2 ** 63 if bits == 64 else int(x) - 2 ** (bits - 1) for x in rng.integers(0, 2 ** bits, 2, dtype=np.uint64, endpoint=False))
        wbits = int(rng.integers(1, 64))
        triples.append((v, o, max(1, int(rng.integers(0, 2 ** wbits, dtype=np.uint64)))))
    got = buckets_of(bucket_exe, triples)
    assert got == [bucket_of(*t) for t in triples]
    assert sum(b is not None and b < 0 for b in got) > 1000 and sum(b is not None and b >= 0 for b in got) > 1000


def test_the_word_keeps_the_order_and_is_never_zero(bucket_exe):
    buckets = [INT64_MIN + 1, -2 ** 62, -65, -64, -1, 0, 1, 63, 64, 2 ** 62, INT64_MAX]
    got = [tuple(int(x) for x in e.split(":")) for e in run_cases(bucket_exe, ["W %d " % len(buckets) + " ".join(map(str, buckets))])[0].split()]
    assert [w for w, _ in got] == [word_of(b) for b in buckets] and [b for _, b in got] == buckets
    assert sorted(w for w, _ in got) == [w for w, _ in got] and all(w != 0 for w, _ in got) and word_of(INT64_MIN) == 0


def check_tables(exe, cases):
    """cases: (words, slots, weak).  The program's slots, loads and table against the restatement's."""
    got = run_cases(exe, ["T %d %d %d %s" % (1 if weak else 0, slots, len(words), " ".join(map(str, words))) for words, slots, weak in cases])
    parsed = []
    for (words, slots, weak), row in zip(cases, got):
        left, right = row.split("|")
        found = [None if s == "full" else int(s) for s, _ in (e.split("@") for e in left.split())]
        loads = [int(l) for _, l in (e.split("@") for e in left.split())]
        table = {int(s): int(w) for s, w in (e.split(":") for e in right.split())}
        want, want_table = probe_words(words, slots, weak)
        assert found == want and table == want_table, (words, slots, weak)
        assert all(1 <= l <= slots for l in loads)
        # one slot per distinct word
        by_word = {}
        for w, s in zip(words, found):
            if s is not None:
                assert by_word.setdefault(w, s) == s and table[s] == w
        parsed.append((found, loads, table))
    return parsed


def test_hash_restated(bucket_exe):
    words = [word_of(b) for b in (INT64_MIN + 1, -1, 0, 1, 2, 64, INT64_MAX)] + [2, M64 - 1]
    for weak in (False, True):
        got = [int(x) for x in run_cases(bucket_exe, ["H %d %d %s" % (weak, len(words), " ".join(map(str, words)))])[0].split()]
        assert got == [bucket_hash(w, weak) for w in words]
        assert (set(got) <= set(range(8))) if weak else (len(set(got)) == len(words))
    # consecutive buckets -- a time-ordered log -- spread over the first slots
    assert len({bucket_hash(word_of(b)) & 1023 for b in range(29_000_000, 29_000_064)}) > 48


def test_seeded_draws_strong_and_weak(bucket_exe):
    cases = []
    for seed in range(6):
        rng = np.random.default_rng(seed)
        distinct = [word_of(int(b)) for b in rng.integers(-2 ** 40, 2 ** 40, 5 + 20 * seed)]
        words = [distinct[int(q)] for q in rng.integers(0, len(distinct), 400)]
        slots = 64
        while slots < 2 * len(set(words)):
            slots *= 2
        cases += [(words, slots, False), (words, slots, True)]
    got = check_tables(bucket_exe, cases)
    assert all(s is not None for found, _, _ in got for s in found)


def test_a_full_table_wraps_around_and_reports_full_after_exactly_n_slots_probes(bucket_exe):
    words = [word_of(b) for b in range(-30, 35)]
    assert len(words) == 65
    full = words[:64]
    for weak in (False, True):
        (f0, l0, t0), (f1, l1, t1), (f2, l2, t2) = check_tables(bucket_exe, [(full, 64, weak), (full + full, 64, weak), (full + [words[64]] + full, 64, weak)])
        assert all(s is not None for s in f0 + f1) and len(t0) == 64 and sorted(f0) == list(range(64))
        assert f2[64] is None and l2[64] == 64                                  # GROUP_NONE after exactly n_slots loaded words
        assert f2[65:] == f0 and t0 == t1 == t2                                 # the 65th left the table as it was
    # the weak hash starts every probe in slots 0 .. 7: word q of 64 wraps nowhere, but a table of 64 words entered from slot 7 on does
    (found, loads, _), = check_tables(bucket_exe, [(full, 64, True)])
    assert max(loads) > 50 and NONE == 0xFFFFFFFF
    # wrap-around proper: words whose first slot is the last one
    last = [w for w in (word_of(b) for b in range(20_000)) if bucket_hash(w) & 63 == 63][:5]
    assert len(last) == 5
    (found, loads, _), = check_tables(bucket_exe, [(last, 64, False)])
    assert found == [63, 0, 1, 2, 3] and loads == [1, 2, 3, 4, 5]


def test_the_digit_plan(bucket_exe):
    pairs = {"one word": (word_of(5), word_of(5)), "bit 0": (word_of(0), word_of(1)), "bit 5": (word_of(0), word_of(32)), "bit 6": (word_of(0), word_of(64)),
             "bit 63": (word_of(-1), word_of(0)), "bit 62": (word_of(0), word_of(2 ** 62)), "bits 59 and 60": (word_of(2 ** 59), word_of(2 ** 60)),
             "the ends": (word_of(INT64_MIN + 1), word_of(INT64_MAX)), "bit 11 / bit 12": (word_of(2 ** 11), word_of(2 ** 12))}
    got = [int(x) for x in run_cases(bucket_exe, ["D %d " % len(pairs) + " ".join("%d %d" % p for p in pairs.values())])[0].split()]
    assert got == [digits_of(*p) for p in pairs.values()]
    assert dict(zip(pairs, got)) == {"one word": 0, "bit 0": 1, "bit 5": 1, "bit 6": 2, "bit 63": 11, "bit 62": 11, "bits 59 and 60": 11, "the ends": 11,
                                     "bit 11 / bit 12": 3}


# ---------------------------------------------------------------------------
# the numpy restatement of the large GPU case against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(0, 0, 1), (1, 0, 1), (300, 0, 60_000), (2000, 123_456, 1000), (2000, 5_000_000, 7), (500, -3, 1)])
def test_the_numpy_restatement_equals_the_oracle_on_small_draws(shape):
    n, origin, width = shape
    v, matched = draw(n, seed=n + width)
    data, offsets, ids, caps = digits_batch(v, matched)
    want = bucket_lines(data, offsets, ids, caps, [(0, 0, -1)], origin, width, [], 1)
    number, first, lines, line_bucket = np_buckets(v, matched, origin, width)
    assert number.tolist() == want["bucket_number"] and first.tolist() == want["first_line"] and lines.tolist() == want["lines"]
    assert line_bucket.tolist() == want["line_bucket"] and want["totals"]["bucketed"] == int(matched.sum()) == want["totals"]["lines"]
    assert n < 2000 or (np.diff(first.astype(np.int64)) < 0).any() or width == 1    # jitter: the first lines are not monotonic
