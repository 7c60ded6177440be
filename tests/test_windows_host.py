"""gx_group_windows / gx_text_group_windows as far as they go without a GPU: the structs, the symbols and the header's text, every
refusal that needs no device, in the order the header states (and "no device is an error, never a CPU path" behind them), that
windows == NULL still checks number_groups and the window, the legality of the size query, the Python side's reading of the window, and
the numpy restatement that the large GPU case is compared with against the oracle (tests/windows_oracle.py) on small random draws of the
same generator."""
import ctypes as C
import os

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError
from windows_oracle import INT64_MAX, INT64_MIN, NONE, WINDOW_FIELDS, draw, group_windows, holds, key_windows, np_windows, wide_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gx_group_windows", "gx_text_group_windows"]
TRIP_OUTPUTS = ("trip_key", "trip_line", "trip_time", "trip_entry", "key_trip_begin")
OTHER_OUTPUTS = ("entry_line", "entry_key", "entry_time", "entry_window_lines", "key_entry_begin", "key_peak_lines", "key_peak_line", "line_window_lines")


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
    O, T, S = N.gx_windows_out, N.gx_windows_totals, None
    assert C.sizeof(O) == 128
    assert [(f, getattr(O, f).offset) for f, _ in O._fields_] == [(name, 8 * q) for q, name in enumerate(
        ("entry_line", "entry_key", "entry_time", "entry_window_lines", "entry_window_sum", "key_entry_begin", "key_peak_lines", "key_peak_line", "line_window_lines",
         "trip_key", "trip_line", "trip_time", "trip_entry", "key_trip_begin", "max_entries", "max_trips"))]
    assert tuple(f for f, _ in O._fields_[:14]) == Gorp.WINDOW_OUTS
    g = C.sizeof(N.gx_group_totals)
    assert C.sizeof(T) == g + 72 and T.group.offset == 0
    assert [(f, getattr(T, f).offset - g) for f, _ in T._fields_[1:]] == [("entries", 0), ("number_unset", 8), ("not_numbers", 16), ("n_trips", 24), ("tripped_keys", 32),
                                                                           ("peak_lines", 40), ("peak_line", 48), ("peak_key", 52), ("first_time", 56), ("last_time", 64)]
    L = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert len(L.gx_group_windows.argtypes) == 18 and len(L.gx_text_group_windows.argtypes) == 17
    header = open(os.path.join(ROOT, "include", "gorp_hip.h")).read()
    body = header[header.index("typedef struct gx_windows_out {"):header.index("} gx_windows_out;")]
    at = [body.index(" " + f + ";") for f, _ in O._fields_]
    assert at == sorted(at)
    body = header[header.index("typedef struct gx_windows_totals {"):header.index("} gx_windows_totals;")]
    assert "gx_group_totals group;" in body and "uint64_t entries, number_unset, not_numbers;" in body and "uint64_t n_trips, tripped_keys;" in body
    assert body.index("peak_lines;") < body.index("peak_line, peak_key;") < body.index("first_time, last_time;")
    body = header[header.index("typedef struct gx_window_sum {"):header.index("} gx_window_sum;")]
    assert body.index("numbers;") < body.index("sum_lo;") < body.index("sum_hi;") < body.index("reserved;")
    for text in NEW + ["while (t - q.peekFirst() > window) q.removeFirst();", "streamstats time_window=60s count by user", "fail2ban's findtime and maxretry",
                       "keyed == entries + number_unset + not_numbers", "window = INT64_MAX still keeps INT64_MIN out\n * of INT64_MAX's window",
                       "the edge, not the level", "HOW THE BATCH IS READ: exactly as gx_group_lines reads it", "With windows == NULL the call IS gx_group_lines",
                       "entries is always a sufficient max_entries and max_trips", "EMPTY INPUTS: n == 0 and n_parts == 0 are legal",
                       "HOST WAITS: TWO host waits before any output", "ONE more wait reads n_trips, tripped_keys and the peak",
                       "NOT IN SCOPE: windows by number of entries (streamstats window=N), centred or leading windows", "state carried from one batch into the next",
                       "73 bytes per entry"]:
        assert text in header, text
    rule = open(os.path.join(ROOT, "gorp_amd", "csrc", "gx_windows.hpp")).read()
    for text in ["Not in scope: windows by number of entries (streamstats window=N)", "GX_WHERE_HD bool window_holds(uint64_t f_word, uint64_t e_word, int64_t window)",
                 "GX_WHERE_HD uint32_t window_lo(", "GX_WHERE_HD bool window_trips(", "GX_WHERE_HD uint64_t window_peak_word(", "struct WindowsDev2"]:
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
    seen = {}

    def both(parts, numbers=(), n_parts=None, numbers_null=False, terms=(), caps_ptr=caps.ctypes.data, flags=0, totals=True, windows=True, outputs=(),
             max_entries=8, max_trips=8, max_keys=8, n=3, window=0, threshold=0, **kw):
        arr = None if parts is None else (N.gx_group_part * max(1, len(parts)))(*parts)
        n_parts = len(parts) if n_parts is None else n_parts
        numbers = list(numbers) + [0] * (n_parts - len(numbers))
        narr = None if numbers_null else (C.c_int32 * max(1, len(numbers)))(*numbers)
        tarr = (N.gx_where_term * max(1, len(terms)))(*terms)
        o = opts(**kw)
        ko = N.gx_group_out()
        ko.max_keys = max_keys
        wo = N.gx_windows_out()
        wo.max_entries, wo.max_trips = max_entries, max_trips
        for name in outputs:
            setattr(wo, name, buf.ctypes.data)
        tot = N.gx_windows_totals()
        tp = C.byref(tot) if totals else None
        wp = C.byref(wo) if windows else None
        rc1 = L.gx_group_windows(g._h.ptr, data.ctypes.data, offsets.ctypes.data, n, ids.ctypes.data, caps_ptr, arr, n_parts, narr, window, threshold, tarr, len(terms),
                                 flags, C.byref(ko), wp, tp, C.byref(o))
        e1 = N.last_error()
        seen["totals"] = Gorp._windows_totals(tot)
        rc2 = L.gx_text_group_windows(g._h.ptr, text.ctypes.data, len(text), arr, n_parts, narr, window, threshold, tarr, len(terms), flags, C.byref(ko), wp, tp, None,
                                      None, C.byref(o))
        e2 = N.last_error()
        return (rc1, e1), (rc2, e2)

    arg = [
        # what gx_group_windows adds
        dict(parts=[part()], numbers_null=True), dict(parts=[part()], numbers=[1]), dict(parts=[part()], numbers=[-2]), dict(parts=[part(extraction=2)], numbers=[3]),
        dict(parts=[part()], window=-1), dict(parts=[], window=-1), dict(parts=[part()], window=INT64_MIN),
        dict(parts=[part()], outputs=("entry_window_sum",)), dict(parts=[], outputs=("entry_window_sum",)),
        dict(parts=[part()], flags=4), dict(parts=[part()], flags=8 | N.GX_BUCKET_ALL_DIGITS), dict(parts=[], flags=0x80000000),
        # gx_group_lines' own
        dict(parts=None, n_parts=1), dict(parts=[part(reserved=1)]),
        dict(parts=[part()], totals=False), dict(parts=[], totals=False),
        dict(parts=[part(extraction=-1)]), dict(parts=[part(extraction=K)]), dict(parts=[part(key_group=1)]), dict(parts=[part(key_group=-1)]),
        dict(parts=[part(extraction=1)]), dict(parts=[part(value_group=1)]), dict(parts=[part(value_group=-2)]), dict(parts=[part(), part()]),
        dict(parts=[part()], terms=[term(extraction=K)]), dict(parts=[part()], terms=[term(group=1)]),
        dict(parts=[part()], utf8=2), dict(parts=[part()], no_sync=1, device_pointers=1),
    ] + [dict(parts=[part()], outputs=(name,)) for name in TRIP_OUTPUTS] + [dict(parts=[], outputs=(name,)) for name in TRIP_OUTPUTS] + [
        dict(parts=[part()], numbers=[-1], threshold=1, outputs=(name,)) for name in TRIP_OUTPUTS + OTHER_OUTPUTS] + [
        dict(parts=[part(), part(extraction=2)], numbers=[-1, -1], outputs=("line_window_lines",))]
    for kw in arg:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG, (kw, msg)
            assert "no CPU fallback" not in msg
    # the order: gx_group_lines' refusals first, then number_groups, the number group, the window, the sums, the trips, outputs without a number
    order = [(dict(parts=[part(key_group=1)], numbers_null=True, window=-1, flags=4), "unknown flag bits"),
             (dict(parts=[part(key_group=1)], numbers_null=True, window=-1), "key_group"),
             (dict(parts=[part()], numbers_null=True, window=-1, outputs=("entry_window_sum", "trip_key")), "number_groups is NULL"),
             (dict(parts=[part()], numbers=[7], window=-1, outputs=("entry_window_sum", "trip_key")), "number group is neither -1 nor one of its extraction's"),
             (dict(parts=[part()], numbers=[-1], window=-1, outputs=("entry_window_sum", "trip_key")), "window below 0"),
             (dict(parts=[part()], numbers=[-1], outputs=("entry_window_sum", "trip_key")), "entry_window_sum without a value_group"),
             (dict(parts=[part()], numbers=[-1], outputs=("trip_key", "entry_line")), "trip outputs with threshold 0"),
             (dict(parts=[part()], numbers=[-1], threshold=3, outputs=("trip_key",), max_entries=2 ** 31), "every part's number group is -1")]
    for kw, words in order:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    # windows == NULL: the call is gx_group_lines, and its own arguments are still checked
    for kw, words in ((dict(parts=[part()], numbers_null=True), "number_groups is NULL"), (dict(parts=[part()], numbers=[5]), "number group"),
                      (dict(parts=[part()], window=-7), "window below 0")):
        for rc, msg in both(windows=False, **kw):
            assert rc == N.GX_E_ARG and words in msg, (kw, msg)
    limit = [dict(parts=[part()], max_entries=2 ** 30 + 1), dict(parts=[part()], max_trips=2 ** 30 + 1), dict(parts=[], max_entries=2 ** 40),
             dict(parts=[], max_trips=2 ** 40), dict(parts=[part()] * 65, numbers=[0] * 65), dict(parts=[part()], max_keys=2 ** 30 + 1)]
    for kw in limit:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_LIMIT, (kw, msg)
    (rc, msg), _ = both(parts=[part()], n=2 ** 32 - 1)
    assert rc == N.GX_E_LIMIT
    (rc, msg), (rc2, _) = both(parts=[part()], caps_ptr=None)
    assert rc == N.GX_E_ARG and "caps" in msg and rc2 == N.GX_E_DEVICE
    # ... and behind all of them: no device is an error, never a CPU path.  Among these the size query (every output NULL, any capacity),
    # trip outputs with a threshold, every other output with threshold 0
    fine = [dict(parts=[]), dict(parts=[], outputs=OTHER_OUTPUTS), dict(parts=[], threshold=2, outputs=OTHER_OUTPUTS + TRIP_OUTPUTS), dict(parts=[], numbers_null=True),
            dict(parts=[part()]), dict(parts=[part()], max_entries=0, max_trips=0), dict(parts=[part()], threshold=5), dict(parts=[part()], outputs=OTHER_OUTPUTS),
            dict(parts=[part()], threshold=1, outputs=OTHER_OUTPUTS + TRIP_OUTPUTS), dict(parts=[part()], threshold=2 ** 32 - 1, outputs=TRIP_OUTPUTS),
            dict(parts=[part()], windows=False), dict(parts=[part()], numbers=[-1]), dict(parts=[part()], numbers=[-1], windows=False),
            dict(parts=[part(value_group=0), part(extraction=2, key_group=1, value_group=0)], numbers=[-1, 2], threshold=2,
                 outputs=OTHER_OUTPUTS + TRIP_OUTPUTS + ("entry_window_sum",)),
            dict(parts=[part(extraction=2, key_group=2, value_group=2)], numbers=[2]),                       # one group may be key, time and value
            dict(parts=[part()], max_entries=2 ** 30, max_trips=2 ** 30),
            dict(parts=[part()], flags=N.GX_GROUP_WEAK_HASH), dict(parts=[part()], flags=N.GX_BUCKET_ALL_DIGITS | N.GX_GROUP_WEAK_HASH),
            dict(parts=[part()], window=INT64_MAX), dict(parts=[part()], terms=[term()]), dict(parts=[part()], utf8=1), dict(parts=[part()], compact_results=2)]
    for kw in fine:
        for rc, msg in both(**kw):
            assert rc == N.GX_E_DEVICE and "no CPU fallback" in msg, (kw, msg)
        t = seen["totals"]
        assert (t["entries"], t["n_trips"], t["peak_lines"], t["peak_line"], t["peak_key"]) == (0, 0, 0, NONE, NONE)
    (rc, msg), _ = both(parts=[part()], utf16=1)
    assert rc == N.GX_E_DEVICE
    # the Python wrappers raise the same
    with pytest.raises(GorpError) as ei:
        g.group_windows(data, offsets, ids, caps, [("gamma", "z", 0)], 60, threshold=5)
    assert ei.value.code == N.GX_E_DEVICE and "no CPU fallback" in ei.value.message
    with pytest.raises(GorpError) as ei:
        g.text_group_windows(bytes(text), [("alpha", "x", "x", "x")], 5, where=[("alpha", "x", "set")])
    assert ei.value.code == N.GX_E_DEVICE


def test_bad_pointers_are_bad_arguments():
    L = N.lib()
    g = three_rules()
    o = opts()
    ids = np.zeros(1, np.int32)
    offsets = np.array([0, 0], np.uint32)
    tot = N.gx_windows_totals()
    for h, off, id_ptr in ((None, offsets.ctypes.data, ids.ctypes.data), (g._h.ptr, None, ids.ctypes.data), (g._h.ptr, offsets.ctypes.data, None)):
        assert L.gx_group_windows(h, None, off, 1, id_ptr, None, None, 0, None, 0, 0, None, 0, 0, None, None, C.byref(tot), C.byref(o)) == N.GX_E_ARG
        assert "bad argument" in N.last_error()
    assert L.gx_text_group_windows(None, None, 0, None, 0, None, 0, 0, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG
    assert L.gx_text_group_windows(g._h.ptr, None, 5, None, 0, None, 0, 0, None, 0, 0, None, None, C.byref(tot), None, None, C.byref(o)) == N.GX_E_ARG


def test_the_window_is_a_number_or_a_text_under_the_first_timed_parts_format():
    g = three_rules()
    both = g.series_parts([("alpha", "x", None), ("gamma", 0, "z")])
    assert g._windows_window(both, 0) == 0 and g._windows_window(both, 60_000) == 60_000 and g._windows_window(both, "45") == 45
    assert g._windows_window(both, INT64_MAX) == INT64_MAX
    for bad in (-1, "-5", "x", 2 ** 63, 1.5, True, None):
        with pytest.raises(ValueError) as ei:
            g._windows_window(both, bad)
        assert "window" in str(ei.value)
    g.set_number_format("gamma", "z", "decimal", 3)
    assert g._windows_window(both, "1.5") == 1500 and g._windows_window(both, 7) == 7


def test_the_rule_of_the_oracle_at_the_corners():
    assert not holds(INT64_MIN, INT64_MAX, INT64_MAX) and holds(-1, INT64_MAX - 1, INT64_MAX) and not holds(-1, INT64_MAX, INT64_MAX)
    assert holds(5, 5, 0) and not holds(5, 6, 0) and holds(-3, 7, 10) and not holds(-3, 8, 10)
    run = lambda times, window, threshold: [(lines, trips) for lines, trips, _, _ in key_windows([(t, i, None) for i, t in enumerate(times)], window, threshold)]
    # the edge, not the level; a key that trips, falls below and trips again
    assert run([0, 1, 2, 3, 50, 51, 52], 10, 3) == [(1, False), (2, False), (3, True), (4, False), (1, False), (2, False), (3, True)]
    assert run([0, 5, 9], 10, 1) == [(1, True), (2, False), (3, False)] and run([0, 5, 9], 10, 0) == [(1, False), (2, False), (3, False)]
    assert run([7, 7, 7], 0, 2) == [(1, False), (2, True), (3, False)]


def test_the_python_dicts_shape_of_the_oracle_on_empty_inputs():
    want = group_windows(np.zeros(0, np.uint8), np.zeros(1, np.uint32), np.zeros(0, np.int32), np.zeros((0, 6), np.int32), [(0, 0, -1, 1)], 5, 2, [], 1)
    assert want["key_entry_begin"] == [0] and want["key_trip_begin"] == [0] and want["line_window_lines"] == [] and want["entry_window_sum"] is None
    assert [want["totals"][k] for k in ("entries", "n_trips", "tripped_keys", "peak_lines", "peak_line", "peak_key")] == [0, 0, 0, 0, NONE, NONE]


@pytest.mark.parametrize("seed", range(6))
def test_the_numpy_restatement_agrees_with_the_oracle_on_small_draws(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    key, t, matched = draw(n, seed, n_keys=int(rng.integers(1, 12)), span=int(rng.integers(2, 40)) * 1000, none=0.2)
    data, offsets, ids, caps = wide_batch(key, t, matched)
    for window, threshold in ((0, 2), (999, 3), (1000, 3), (3000, 1), (3000, 0), (INT64_MAX, 4), (10 ** 6, 2 ** 32 - 1)):
        want = group_windows(data, offsets, ids, caps, [(0, 0, -1, 1)], window, threshold, [], 1)
        got = np_windows(key, t, matched, window, threshold)
        for name, dtype in WINDOW_FIELDS:
            assert got[name].dtype == dtype and got[name].tolist() == want[name], (name, window, threshold)
        for name, value in got["totals"].items():
            assert value == want["totals"][name], (name, window, threshold)
    # nothing matched at all
    got = np_windows(key, t, np.zeros(n, bool), 5, 2)
    want = group_windows(data, offsets, np.full(n, -1, np.int32), caps, [(0, 0, -1, 1)], 5, 2, [], 1)
    for name, _ in WINDOW_FIELDS:
        assert got[name].tolist() == want[name], name
    assert got["totals"]["peak_line"] == NONE == want["totals"]["peak_line"]
