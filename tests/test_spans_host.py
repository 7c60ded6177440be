"""gx_group_spans / gx_text_group_spans as far as they go without a GPU: the structs, the symbols and the header's text, every refusal
that needs no device, in the order the header states (and "no device is an error, never a CPU path" behind them), that spans == NULL
still checks number_groups and roles, the Python side's reading of the parts, and the numpy restatement that the large GPU case is
compared with against the oracle (tests/spans_oracle.py: the put / remove loop) on small random draws of the same generator."""
import ctypes as C
import os

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from spans_oracle import BEGIN, END, INT64_MAX, INT64_MIN, SPAN_FIELDS, batch, draw, duration, group_spans, identities, np_spans, wide_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_spans", "gx_text_group_spans"]


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


def test_struct_layouts_symbols_and_header_text():
    O, T = N.gx_spans_out, N.gx_spans_totals
    assert C.sizeof(O) == 104
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("span_key", 0), ("span_begin_line", 8), ("span_end_line", 16), ("span_begin", 24), ("span_end", 32),
                                                                    ("span_duration", 40), ("span_class", 48), ("key_span_begin", 56), ("key_span_stats", 64),
                                                                    ("key_open_line", 72), ("line_span", 80), ("line_state", 88), ("max_spans", 96)]
    g = C.sizeof(N.gx_group_totals)
    assert C.sizeof(T) == g + 120 and T.group.offset == 0
    assert [(f, getattr(T, f).offset - g) for f, _ in T._fields_[1:]] == [("n_spans", 0), ("begins", 8), ("ends", 16), ("superseded", 24), ("left_open", 32),
                                                                           ("orphan_ends", 40), ("out_of_range", 48), ("durations", 56)]
    assert (N.GX_SPAN_BEGIN, N.GX_SPAN_END) == (BEGIN, END) == (1, 2)
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert len(L.gx_group_spans.argtypes) == 17 and len(L.gx_text_group_spans.argtypes) == 16
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    body = header[header.index("typedef struct gx_spans_out {"):header.index("} gx_spans_out;")]
    at = [body.index(" " + f + ";") for f, _ in O._fields_]
    assert at == sorted(at)
    body = header[header.index("typedef struct gx_spans_totals {"):header.index("} gx_spans_totals;")]
    assert "gx_group_totals group;" in body and "uint64_t n_spans, begins, ends, superseded, left_open, orphan_ends, out_of_range;" in body
    assert "gx_measure_stats durations;" in body
    for text in NEW + ["#define GX_SPAN_BEGIN 1u", "#define GX_SPAN_END   2u", "transaction id startswith=... endswith=...", "prev = open.put(id(r), r)",
                       "b = open.remove(id(r))", "if and only if that\n * entry is a BEGIN", "because put replaces and remove empties",
                       "keyed == begins + ends; begins == n_spans + superseded + left_open; ends == n_spans + orphan_ends",
                       "out_of_range <= durations.not_numbers", "HOW THE BATCH IS READ: exactly as gx_group_lines reads it",
                       "With spans == NULL the call IS gx_group_lines", "EMPTY INPUTS: n == 0 and n_parts == 0 are legal", "HOST WAITS: TWO host waits before any output",
                       "ONE more wait reads n_spans", "NOT IN SCOPE: pairing in time order", "quantiles of durations, ranking spans",
                       "18 bytes per input line; 98 bytes per entry"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_spans.hpp")).read()
    for text in ["Not in scope: pairing in time order", "GX_WHERE_HD bool span_duration(int64_t begin, int64_t end, int64_t* duration)",
                 "GX_WHERE_HD uint32_t span_state(", "struct SpansHead", "struct SpansDev"]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule and "__int128" not in rule and "double" not in rule and "float" not in rule


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    return N.gx_group_part(extraction, key_group, value_group, reserved)


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


EVERY_OUTPUT = ("span_key", "span_begin_line", "span_end_line", "span_begin", "span_end", "span_duration", "span_class", "key_span_begin", "key_span_stats",
                "key_open_line", "line_span", "line_state")


def test_every_refusal_comes_before_the_look_at_the_device_in_order():
    L = N.lib()
    g = three_rules()          # K = 3; groups: alpha 1, beta 0, gamma 3
    K = 3
    ids = np.array([0, -1, 2], np.int32)
    caps = np.full((3, 6), -1, np.int32)
    data = np.frombuffer(b"abczzd1", dtype=np.uint8)
    offsets = np.array([0, 2, 5, 7], np.uint32)
    text = np.frombuffer(b"ab\nzz\nd1\n", dtype=np.uint8)
    buf = np.zeros(64, np.uint64)

    def both(parts, numbers=(), roles=(), n_parts=None, numbers_null=False, roles_null=False, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, spans=True,
             outputs=(), max_spans=8, max_keys=8, n=3, **kw):
        arr = None if parts is None else (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        numbers = list(numbers) + [0] * (n_parts - len(numbers))
        roles = list(roles) + [BEGIN] * (n_parts - len(roles))
        narr = None if numbers_null else (C.c_int32 * max(1, len(numbers)))(*numbers)
        rarr = None if roles_null else (C.c_uint32 * max(1, len(roles)))(*roles)
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        ko = N.gx_group_out()
        ko.max_keys = max_keys
        so = N.gx_spans_out()
        so.max_spans = max_spans
        for name in outputs:
            setattr(so, name, buf.ctypes.data)
        tot = N.gx_spans_totals()
        tp = C.byref(tot) if totals else None
        sp = C.byref(so) if spans else None
        rc1 = L.gx_group_spans(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, narr, rarr, tarr, len(terms), flags,
                               C.byref(ko), sp, tp, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_spans(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, narr, rarr, tarr, len(terms), flags, C.byref(ko), sp, tp, None, None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        # what gx_group_spans adds
        dict(parts=[part()], numbers_null=True), dict(parts=[part()], numbers=[1]), dict(parts=[part()], numbers=[-2]), dict(parts=[part(extraction=2)], numbers=[3]),
        dict(parts=[part()], roles_null=True), dict(parts=[part()], roles=[0]), dict(parts=[part()], roles=[3]), dict(parts=[part()], roles=[0xFFFFFFFF]),
        dict(parts=[part(), part(extraction=2)], roles=[END, 4]),
        dict(parts=[part()], flags=4), dict(parts=[part()], flags=8 | N.GX_BY_KEY_ALL_DIGITS), dict(parts=[], flags=0x80000000),
        # gx_group_lines' own
        dict(parts=None, n_parts=1), dict(parts=[part(reserved=1)]),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]),
        dict(parts=[part(extraction=1)]), dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(), part()]),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    # the order: gx_group_lines' refusals first, then number_groups, the number group, roles, the role
    order = [(dict(parts=[part(key_group=1)], numbers_null=True, roles_null=True, flags=4), "unknown flag bits"),
             (dict(parts=[part(key_group=1)], numbers_null=True, roles_null=True), "key_group"),
             (dict(parts=[part()], numbers_null=True, roles_null=True), "number_groups is NULL"),
             (dict(parts=[part()], numbers=[7], roles_null=True), "number group is neither -1 nor one of its extraction's"),
             (dict(parts=[part()], numbers=[-1], roles_null=True, max_spans=2 ** 31), "roles is NULL"),
             (dict(parts=[part()], numbers=[-1], roles=[5], max_spans=2 ** 31), "role is neither GX_SPAN_BEGIN nor GX_SPAN_END")]
    for kw, words in order:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    # spans == NULL: the call is gx_group_lines, and its own arguments are still checked
    for kw, words in ((dict(parts=[part()], numbers_null=True), "number_groups is NULL"), (dict(parts=[part()], numbers=[5]), "number group"),
                      (dict(parts=[part()], roles_null=True), "roles is NULL"), (dict(parts=[part()], roles=[7]), "role is neither")):
        for rc, msg in both(spans=False, **kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    limit = [dict(parts=[part()], max_spans=2 ** 30 + 1), dict(parts=[], max_spans=2 ** 40), dict(parts=[part()] * 65, numbers=[0] * 65),
             dict(parts=[part()], max_keys=2 ** 30 + 1)]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[], outputs=EVERY_OUTPUT), dict(parts=[], numbers_null=True, roles_null=True), dict(parts=[part()]),
            dict(parts=[part()], outputs=EVERY_OUTPUT), dict(parts=[part()], spans=False), dict(parts=[part()], roles=[END]),
            dict(parts=[part()], numbers=[-1], outputs=EVERY_OUTPUT),                                        # durations without a time: legal, every span class 1
            dict(parts=[part()], numbers=[-1], spans=False),
            dict(parts=[part(value_group=0), part(extraction=2, key_group=1, value_group=0)], numbers=[-1, 2], roles=[BEGIN, END], outputs=EVERY_OUTPUT),
            dict(parts=[part(extraction=2, key_group=2, value_group=2)], numbers=[2]),                       # one group may be key, time and value
            dict(parts=[part()], max_spans=0), dict(parts=[part()], max_spans=2 ** 30),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BY_KEY_ALL_DIGITS | N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_spans(data, offsets, ids, caps, [("gamma", "z", 0, "begin"), ("alpha", "x", None, "end")])
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_spans(bytes(text), [("alpha", "x", "x", "end", "x")], where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_spans_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_spans(h, None, off, 1, id_ptr, None, None, 0, None, None, None, 0, 0, None, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_spans(None, None, 0, None, 0, None, None, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_group_spans(g._h.ptr, None, 5, None, 0, None, None, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_span_parts_reads_names_indices_roles_and_no_time():
    g = three_rules()
    p, numbers, roles = g.span_parts([("alpha", "x", None, "begin"), ("gamma", 0, "z", "end", 1)])
    assert p.n == 2 and (p.array[0].extraction, p.array[0].key_group, p.array[0].value_group) == (0, 0, -1)
    assert (p.array[1].extraction, p.array[1].key_group, p.array[1].value_group) == (2, 0, 1)
    assert list(numbers)[:2] == [-1, 2] and list(roles)[:2] == [N.GX_SPAN_BEGIN, N.GX_SPAN_END]
    assert g.span_parts((p, numbers, roles)) == (p, numbers, roles)
    assert list(g.span_parts([(0, 0, 0, N.GX_SPAN_END)])[2])[:1] == [N.GX_SPAN_END]
    for bad in ([("alpha", "x", None)], [("alpha", "x", None, "middle")], [("alpha", "x", None, 0)], [("alpha", "x", None, "begin", "x", "x")]):
        with pytest.raises(ValueError):
            g.span_parts(bad)


def test_the_duration_of_the_oracle_at_the_corners():
    # (out of range: the sides stay the numbers they are, the duration is 0 and the class 2)
    assert duration(0, INT64_MIN, 0, INT64_MAX) == (2, INT64_MIN, INT64_MAX, 0, True) and duration(0, INT64_MAX, 0, INT64_MIN) == (2, INT64_MAX, INT64_MIN, 0, True)
    assert duration(0, -1, 0, INT64_MAX) == (2, -1, INT64_MAX, 0, True) and duration(0, 0, 0, INT64_MAX) == (0, 0, INT64_MAX, INT64_MAX, False)   # 2^63 and 2^63 - 1
    assert duration(0, 0, 0, INT64_MIN) == (0, 0, INT64_MIN, INT64_MIN, False) and duration(0, INT64_MIN, 0, -1) == (0, INT64_MIN, -1, INT64_MAX, False)
    assert duration(0, 5, 0, 5) == (0, 5, 5, 0, False) and duration(0, 9, 0, 2) == (0, 9, 2, -7, False)
    assert duration(1, 0, 0, 7) == (1, 0, 7, 0, False) and duration(0, 7, 2, 0) == (2, 7, 0, 0, False) and duration(1, 0, 2, 0) == (2, 0, 0, 0, False)


def test_b_b_e_e_in_the_oracle():
    data, offsets, ids, caps = batch([b"k"] * 4, [1, 2, 5, 9], ids=[0, 0, 1, 1])
    got = group_spans(data, offsets, ids, caps, [(0, 0, -1, 1, BEGIN), (1, 0, -1, 1, END)], [], 2)
    assert got["line_state"] == [3, 1, 2, 5] and got["span_begin_line"] == [1] and got["span_end_line"] == [2] and got["span_duration"] == [3]
    assert identities(got["totals"]) and got["key_open_line"] == [0xFFFFFFFF]


@pytest.mark.parametrize("seed", range(8))
def test_the_numpy_restatement_agrees_with_the_oracle_on_small_draws(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 500))
    key, role, t, matched = draw(n, seed, n_keys=int(rng.integers(1, 12)), span=int(rng.integers(2, 40)) * 1000, none=0.2, begin=float(rng.uniform(0.2, 0.8)))
    data, offsets, ids, caps = wide_batch(key, role, t, matched)
    parts = [(0, 0, -1, 1, BEGIN), (1, 0, -1, 1, END)]
    want = group_spans(data, offsets, ids, caps, parts, [], 2)
    got = np_spans(key, role, t, matched)
    for name, dtype in SPAN_FIELDS:
        assert got[name].dtype == dtype and got[name].tolist() == want[name], name
    assert identities(want["totals"])
    # nothing matched at all
    got = np_spans(key, role, t, np.zeros(n, bool))
    want = group_spans(data, offsets, np.full(n, -1, np.int32), caps, parts, [], 2)
    for name, _ in SPAN_FIELDS:
        assert got[name].tolist() == want[name], name
