"""gx_group_sessions / gx_text_group_sessions as far as they go without a GPU: the structs, the symbols and the header's text, every
refusal that needs no device, in the order the header states (and "no device is an error, never a CPU path" behind them), that
sessions == NULL still checks number_groups and max_gap, the Python side's reading of max_gap, and the numpy restatement that the large
GPU case is compared with against the oracle (tests/sessions_oracle.py) on small random draws of the same generator."""
import ctypes as C
import os

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from sessions_oracle import INT64_MAX, INT64_MIN, SESSION_FIELDS, draw, group_sessions, np_sessions, opens, wide_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_sessions", "gx_text_group_sessions"]


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
    O, T = N.gx_sessions_out, N.gx_sessions_totals
    assert C.sizeof(O) == 96
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [("session_key", 0), ("session_begin", 8), ("session_end", 16), ("session_first_line", 24),
                                                                    ("session_lines", 32), ("session_stats", 40), ("session_entry_begin", 48), ("key_session_begin", 56),
                                                                    ("entry_line", 64), ("line_session", 72), ("max_sessions", 80), ("max_entries", 88)]
    g = C.sizeof(N.gx_group_totals)
    assert C.sizeof(T) == g + 64 and T.group.offset == 0
    assert [(f, getattr(T, f).offset - g) for f, _ in T._fields_[1:]] == [("n_sessions", 0), ("entries", 8), ("number_unset", 16), ("not_numbers", 24),
                                                                           ("longest_lines", 32), ("longest_duration", 40), ("first_time", 48), ("last_time", 56)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert len(L.gx_group_sessions.argtypes) == 17 and len(L.gx_text_group_sessions.argtypes) == 16
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    # the structs' fields in the header, in the order of the ctypes structs
    body = header[header.index("typedef struct gx_sessions_out {"):header.index("} gx_sessions_out;")]
    at = [body.index(" " + f + ";") for f, _ in O._fields_]
    assert at == sorted(at)
    body = header[header.index("typedef struct gx_sessions_totals {"):header.index("} gx_sessions_totals;")]
    assert "gx_group_totals group;" in body and "uint64_t n_sessions, entries, number_unset, not_numbers;" in body
    assert body.index("longest_lines;") < body.index("longest_duration;") < body.index("first_time, last_time;")
    for text in NEW + ["byId.computeIfAbsent(r.asMap().get(\"id\"), k -> new ArrayList<>()).add(r);", "transaction id maxpause=30s",
                       "keyed == entries + number_unset + not_numbers", "max_gap = INT64_MAX still splits INT64_MIN from INT64_MAX",
                       "Equal times never open a\n * session", "HOW THE BATCH IS READ: exactly as gx_group_lines reads it",
                       "With sessions == NULL the call IS gx_group_lines", "entries is always a sufficient max_sessions and max_entries",
                       "EMPTY INPUTS: n == 0 and n_parts == 0 are legal", "HOST WAITS: TWO host waits before any output", "ONE more wait reads n_sessions",
                       "NOT IN SCOPE: a cap on a session's span (maxspan), start / end markers (startswith)", "quantiles\n * of durations, ranking sessions",
                       "17 bytes per input line (26 with a value group); 65 bytes per entry"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_sessions.hpp")).read()
    for text in ["Not in scope: a cap on a session's span (maxspan)", "GX_WHERE_HD bool session_opens(uint64_t gap, int64_t max_gap)", "struct SessionsHead",
                 "struct SessionsDev", "struct SessionsDev2"]:
        assert text in rule, text
    assert "hip_runtime" not in rule and "__global__" not in rule and "__int128" not in rule and "double" not in rule and "float" not in rule


def part(extraction=0, key_group=0, value_group=-1, reserved=0):
    return N.gx_group_part(extraction, key_group, value_group, reserved)


def term(extraction=0, group=0, op=N.GX_WHERE_SET, text_units=0):
    t = N.gx_where_term()
    t.extraction, t.group, t.op, t.text_units = extraction, group, op, text_units
    return t


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

    def both(parts, numbers=(), n_parts=None, numbers_null=False, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, sessions=True, outputs=(),
             max_sessions=8, max_keys=8, n=3, max_gap=0, **kw):
        arr = None if parts is None else (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        numbers = list(numbers) + [0] * (n_parts - len(numbers))
        narr = None if numbers_null else (C.c_int32 * max(1, len(numbers)))(*numbers)
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        ko = N.gx_group_out()
        ko.max_keys = max_keys
        so = N.gx_sessions_out()
        so.max_sessions, so.max_entries = max_sessions, 8
        for name in outputs:
            setattr(so, name, buf.ctypes.data)
        tot = N.gx_sessions_totals()
        tp = C.byref(tot) if totals else None
        sp = C.byref(so) if sessions else None
        rc1 = L.gx_group_sessions(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, narr, max_gap, tarr, len(terms), flags,
                                  C.byref(ko), sp, tp, C.byref(o))
        e1 = N.last_error()
        rc2 = L.gx_text_group_sessions(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, narr, max_gap, tarr, len(terms), flags, C.byref(ko), sp, tp, None, None,
                                       C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    every_output = ("session_key", "session_begin", "session_end", "session_first_line", "session_lines", "session_entry_begin", "key_session_begin", "entry_line",
                    "line_session")
    arg = [
        # what gx_group_sessions adds
        dict(parts=[part()], numbers_null=True), dict(parts=[part()], numbers=[1]), dict(parts=[part()], numbers=[-2]), dict(parts=[part(extraction=2)], numbers=[3]),
        dict(parts=[part()], max_gap=-1), dict(parts=[], max_gap=-1), dict(parts=[part()], max_gap=INT64_MIN),
        dict(parts=[part()], outputs=("session_stats",)), dict(parts=[], outputs=("session_stats",)),
        dict(parts=[part()], flags=4), dict(parts=[part()], flags=8 | N.GX_BUCKET_ALL_DIGITS), dict(parts=[], flags=0x80000000),
        # gx_group_lines' own
        dict(parts=None, n_parts=1), dict(parts=[part(reserved=1)]),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]),
        dict(parts=[part(extraction=1)]), dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(), part()]),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ] + [dict(parts=[part()], numbers=[-1], outputs=(name,)) for name in every_output] + [
        dict(parts=[part(), part(extraction=2)], numbers=[-1, -1], outputs=("line_session",))]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    # the order: gx_group_lines' refusals first, then number_groups, the number group, max_gap, session_stats, outputs without a number
    order = [(dict(parts=[part(key_group=1)], numbers_null=True, max_gap=-1, flags=4), "unknown flag bits"),
             (dict(parts=[part(key_group=1)], numbers_null=True, max_gap=-1), "key_group"),
             (dict(parts=[part()], numbers_null=True, max_gap=-1, outputs=("session_stats",)), "number_groups is NULL"),
             (dict(parts=[part()], numbers=[7], max_gap=-1, outputs=("session_stats",)), "number group is neither -1 nor one of its extraction's"),
             (dict(parts=[part()], numbers=[-1], max_gap=-1, outputs=("session_stats",)), "max_gap below 0"),
             (dict(parts=[part()], numbers=[-1], outputs=("session_stats", "session_key")), "session_stats without a value_group"),
             (dict(parts=[part()], numbers=[-1], outputs=("session_key",), max_sessions=2 ** 31), "every part's number group is -1")]
    for kw, words in order:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    # sessions == NULL: the call is gx_group_lines, and its own arguments are still checked
    for kw, words in ((dict(parts=[part()], numbers_null=True), "number_groups is NULL"), (dict(parts=[part()], numbers=[5]), "number group"),
                      (dict(parts=[part()], max_gap=-7), "max_gap below 0")):
        for rc, msg in both(sessions=False, **kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    limit = [dict(parts=[part()], max_sessions=2 ** 30 + 1), dict(parts=[], max_sessions=2 ** 40), dict(parts=[part()] * 65, numbers=[0] * 65),
             dict(parts=[part()], max_keys=2 ** 30 + 1)]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path
    fine = [dict(parts=[]), dict(parts=[], outputs=every_output), dict(parts=[], numbers_null=True), dict(parts=[part()]), dict(parts=[part()], outputs=every_output),
            dict(parts=[part()], sessions=False), dict(parts=[part()], numbers=[-1]), dict(parts=[part()], numbers=[-1], sessions=False),
            dict(parts=[part(value_group=0), part(extraction=2, key_group=1, value_group=0)], numbers=[-1, 2], outputs=every_output + ("session_stats",)),
            dict(parts=[part(extraction=2, key_group=2, value_group=2)], numbers=[2]),                       # one group may be key, time and value
            dict(parts=[part()], max_sessions=0), dict(parts=[part()], max_sessions=2 ** 30),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BUCKET_ALL_DIGITS | N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], max_gap=INT64_MAX), dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_sessions(data, offsets, ids, caps, [("gamma", "z", 0)], 60)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_sessions(bytes(text), [("alpha", "x", "x", "x")], 5, where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_sessions_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_sessions(h, None, off, 1, id_ptr, None, None, 0, None, 0, None, 0, 0, None, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_sessions(None, None, 0, None, 0, None, 0, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_group_sessions(g._h.ptr, None, 5, None, 0, None, 0, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_max_gap_is_a_number_or_a_text_under_the_first_timed_parts_format():
    g = three_rules()
    both = g.series_parts([("alpha", "x", None), ("gamma", 0, "z")])
    assert g._sessions_gap(both, 0) == 0 and g._sessions_gap(both, 30_000) == 30_000 and g._sessions_gap(both, "45") == 45
    assert g._sessions_gap(both, INT64_MAX) == INT64_MAX
    for bad in (-1, "-5", "x", 2 ** 63, 1.5, True, None):
        with pytest.raises(ValueError):
            g._sessions_gap(both, bad)
    g.set_number_format("gamma", "z", "decimal", 3)
    assert g._sessions_gap(both, "1.5") == 1500 and g._sessions_gap(both, 7) == 7


def test_the_gap_rule_of_the_oracle_at_the_corners():
    assert opens(INT64_MIN, INT64_MAX, INT64_MAX) and not opens(5, 5, 0) and opens(5, 6, 0) and not opens(-3, 7, 10) and opens(-3, 8, 10)


@pytest.mark.parametrize("seed", range(6))
def test_the_numpy_restatement_agrees_with_the_oracle_on_small_draws(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    key, t, matched = draw(n, seed, n_keys=int(rng.integers(1, 12)), span=int(rng.integers(2, 40)) * 1000, none=0.2)
    data, offsets, ids, caps = wide_batch(key, t, matched)
    for max_gap in (0, 999, 1000, 3000, INT64_MAX):
        want = group_sessions(data, offsets, ids, caps, [(0, 0, -1, 1)], max_gap, [], 1)
        got = np_sessions(key, t, matched, max_gap)
        for name, dtype in SESSION_FIELDS:
            assert got[name].dtype == dtype and got[name].tolist() == want[name], (name, max_gap)
    # nothing matched at all
    got = np_sessions(key, t, np.zeros(n, bool), 5)
    want = group_sessions(data, offsets, np.full(n, -1, np.int32), caps, [(0, 0, -1, 1)], 5, [], 1)
    for name, _ in SESSION_FIELDS:
        assert got[name].tolist() == want[name], name
