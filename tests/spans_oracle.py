"""The rule of gx_group_spans restated in Python, for the tests of both sides (tests/test_spans_host.py; tests/test_gpu_spans.py: the
kernels), as the loop the reference's caller writes: a line counts when its outcome is an extraction that has a part and every term of
that extraction holds (where_oracle.keep_lines); it is keyed when its key group names a value (where_oracle.pair_set); every keyed line
is an entry whose role is its part's, and ONE pass over the lines in input order keeps a dict `open` of the begin that is open per key:
a BEGIN puts itself there and supersedes what was there, an END removes what is there and forms a span with it, or is an orphan; what
is left in `open` at the end was never finished.  A side's time is sliced out of the line with the capture offsets and parsed under its
format (number_oracle.parse); the durations are differences of Python's integers: nothing can overflow.  The spans are sorted by (key
number, end line) at the end.  Deliberately NOT the sorted-neighbour formulation the kernels use; np_spans below is that one, for the
large shape."""
import numpy as np

from bucket_oracle import INT64_MAX, INT64_MIN, NONE, summarise
from number_oracle import LONG, parse
from series_oracle import batch
from where_oracle import keep_lines, outcome, pair_set, unpack

assert (INT64_MIN, INT64_MAX, NONE) == (-2 ** 63, 2 ** 63 - 1, 0xFFFFFFFF) and batch

BEGIN, END = 1, 2
S_NONE, S_BEGIN, S_END, S_SUPERSEDED, S_OPEN, S_ORPHAN = range(6)
SPAN_FIELDS = (("span_key", np.uint32), ("span_begin_line", np.uint32), ("span_end_line", np.uint32), ("span_begin", np.int64), ("span_end", np.int64),
               ("span_duration", np.int64), ("span_class", np.uint8), ("key_span_begin", np.uint64), ("key_open_line", np.uint32), ("line_span", np.uint32),
               ("line_state", np.uint8))
SPAN_TOTALS = ("n_spans", "begins", "ends", "superseded", "left_open", "orphan_ends", "out_of_range")


def decode_parts(three):
    """Gorp.span_parts' result as [(extraction, key group, value group or -1, number group or -1, role)]."""
    p, numbers, roles = three
    return [(p.array[t].extraction, p.array[t].key_group, p.array[t].value_group, numbers[t], roles[t]) for t in range(p.n)]


def duration(cb, b, ce, e):
    """(class, begin, end, duration, out of range) of a span from its sides' (class, time): Python's integers"""
    cls = max(cb, ce)
    oor = False
    d = 0
    if cls == 0:
        d = e - b
        if not INT64_MIN <= d <= INT64_MAX:
            cls, d, oor = 2, 0, True
    return cls, (b if cb == 0 else 0), (e if ce == 0 else 0), d, oor


def group_spans(data, offsets, ids, caps, parts, terms, K, formats=None):
    """What gx_group_spans delivers beside gx_group_lines' outputs, and the group totals it rests on.  ids: int32 match ids and caps
    their dense rows, or ids = u16 / u8 result rows (caps None); parts: decode_parts'; terms: where_oracle.decode_terms'; formats:
    {(extraction, group): (kind, scale)}, LONG where absent."""
    formats = formats or {}
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    by_k = {k: (kg, ng, role) for k, kg, _, ng, role in parts}
    counted = np.isin(oc, list(by_k))
    keep = np.zeros(len(oc), bool)
    if counted.any():
        keep[counted] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[counted] if terms else True

    def text(i, g):
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        return data[off[i] + b:off[i] + e] if pair_set(b, e, off[i + 1] - off[i]) else None

    def number(i, g):
        """(class, value): 0 a number, 1 unset, 2 no number"""
        t = text(i, g)
        if t is None:
            return 1, 0
        v = parse(*formats.get((int(oc[i]), g), (LONG, 0)), t.tolist())
        return (2, 0) if v is None else (0, v)

    n = len(oc)
    key_number, open_ = {}, {}
    totals = {"lines": int(keep.sum()), "keyed": 0, "unset": 0, "begins": 0, "ends": 0, "superseded": 0, "orphan_ends": 0}
    state = [S_NONE] * n
    spans = []
    for i in range(n):
        if not keep[i]:
            continue
        kg, ng, role = by_k[int(oc[i])]
        key = text(i, kg)
        if key is None:
            totals["unset"] += 1
            continue
        totals["keyed"] += 1
        j = key_number.setdefault((key.dtype.itemsize, key.tobytes()), len(key_number))
        r = (i, number(i, ng) if ng >= 0 else (1, 0))
        if role == BEGIN:
            totals["begins"] += 1
            prev = open_.get(j)
            open_[j] = r                                           # open.put(id, r)
            if prev is not None:
                totals["superseded"] += 1
                state[prev[0]] = S_SUPERSEDED
        else:
            totals["ends"] += 1
            b = open_.pop(j, None)                                 # open.remove(id)
            if b is None:
                totals["orphan_ends"] += 1
                state[i] = S_ORPHAN
            else:
                state[b[0]], state[i] = S_BEGIN, S_END
                spans.append((j, i, b[0]) + duration(*b[1], *r[1]))
    key_open = [NONE] * len(key_number)
    for j, (i, _) in open_.items():
        state[i] = S_OPEN
        key_open[j] = i
    spans.sort(key=lambda s: (s[0], s[1]))
    line_span = [NONE] * n
    for s, row in enumerate(spans):
        line_span[row[1]] = line_span[row[2]] = s
    skey = [row[0] for row in spans]
    stats_of = lambda rows: summarise([r[6] for r in rows if r[3] == 0], sum(r[3] == 1 for r in rows), sum(r[3] == 2 for r in rows))
    per_key = [[] for _ in key_number]
    for row in spans:
        per_key[row[0]].append(row)
    totals.update(n_keys=len(key_number), n_spans=len(spans), left_open=len(open_), out_of_range=sum(row[7] for row in spans), durations=stats_of(spans))
    return {"span_key": skey, "span_begin_line": [row[2] for row in spans], "span_end_line": [row[1] for row in spans], "span_begin": [row[4] for row in spans],
            "span_end": [row[5] for row in spans], "span_duration": [row[6] for row in spans], "span_class": [row[3] for row in spans],
            "key_span_begin": np.searchsorted(np.asarray(skey, np.int64), np.arange(len(key_number) + 1)).tolist(), "key_span_stats": [stats_of(rows) for rows in per_key],
            "key_open_line": key_open, "line_span": line_span, "line_state": state, "totals": totals, "keys": [k[1] for k in key_number]}


def identities(t):
    """the identities include/gorp_hip.h states, on a totals dict"""
    assert t["keyed"] == t["begins"] + t["ends"], t
    assert t["begins"] == t["n_spans"] + t["superseded"] + t["left_open"], t
    assert t["ends"] == t["n_spans"] + t["orphan_ends"], t
    assert t["durations"]["lines"] == t["n_spans"] and t["out_of_range"] <= t["durations"]["not_numbers"], t
    return True


def same(got, want):
    """Gorp.group_spans' dict against group_spans': every span field and total, bit for bit."""
    t, g = want["totals"], got["totals"]
    for name in t:
        assert g[name] == t[name], (name, g[name], t[name])
    for name, dtype in SPAN_FIELDS:
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    assert len(got["key_span_stats"]) == len(want["key_span_stats"])
    for j, (a, b) in enumerate(zip(got["key_span_stats"], want["key_span_stats"])):
        assert a == b, (j, a, b)
    return identities(g)


# ---------------------------------------------------------------------------
# the large shape: key numbers, roles and times as arrays, the batch written by numpy alone, and the restatement by a stable argsort by
# key number and shifted compares -- the formulation the kernels use
# ---------------------------------------------------------------------------
KEY_DIGITS, TIME_DIGITS = 5, 10


def draw(n, seed, n_keys=4000, span=3_000_000_000, none=0.03, begin=0.5):
    """n (key, role, time) lines: the roles drawn at random, so every state occurs; a share of lines that match nothing"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, n_keys, n).astype(np.int64), np.where(rng.random(n) < begin, BEGIN, END).astype(np.int64), rng.integers(0, span, n).astype(np.int64),
            rng.random(n) >= none)


def wide_batch(key, role, t, matched):
    """every line is its key in KEY_DIGITS decimal digits, its time in TIME_DIGITS, zero-padded, and one byte of filler; extraction 0 the
    BEGIN lines, extraction 1 the END lines"""
    n = len(t)
    w = KEY_DIGITS + TIME_DIGITS + 1
    data = np.full((n, w), 0x2E, np.uint8)
    q = key.copy()
    for d in range(KEY_DIGITS - 1, -1, -1):
        data[:, d] = 48 + q % 10
        q //= 10
    q = t.copy()
    for d in range(KEY_DIGITS + TIME_DIGITS - 1, KEY_DIGITS - 1, -1):
        data[:, d] = 48 + q % 10
        q //= 10
    offsets = (np.arange(n + 1, dtype=np.int64) * w).astype(np.uint32)
    caps = np.tile(np.array([0, KEY_DIGITS, KEY_DIGITS, KEY_DIGITS + TIME_DIGITS, -1, -1], np.int32), (n, 1))
    return data.reshape(-1), offsets, np.where(matched, role - 1, -1).astype(np.int32), caps


def np_spans(key, role, t, matched):
    """{field: array}: key numbers by first appearance, a stable argsort by key number, the states by compares with the neighbours"""
    n = len(t)
    at = np.flatnonzero(matched)
    names, first = np.unique(key[at], return_index=True)
    number_of = np.zeros(int(names.max()) + 1 if len(names) else 1, np.int64)
    number_of[names[np.argsort(first)]] = np.arange(len(names))
    kn = number_of[key[at]]
    order = np.argsort(kn, kind="stable")
    kn, line, r, tt = kn[order], at[order], role[at][order], t[at][order]
    m = len(at)
    prev_same = np.concatenate([[False], kn[1:] == kn[:-1]]) if m else np.zeros(0, bool)
    next_same = np.concatenate([kn[1:] == kn[:-1], [False]]) if m else np.zeros(0, bool)
    prev_role = np.concatenate([[0], r[:-1]]) if m else r
    next_role = np.concatenate([r[1:], [0]]) if m else r
    state = np.where(r == BEGIN, np.where(~next_same, S_OPEN, np.where(next_role == END, S_BEGIN, S_SUPERSEDED)),
                     np.where(prev_same & (prev_role == BEGIN), S_END, S_ORPHAN))
    ends = np.flatnonzero(state == S_END)
    line_state = np.zeros(n, np.uint8)
    line_state[line] = state
    line_span = np.full(n, NONE, np.uint32)
    line_span[line[ends]] = np.arange(len(ends))
    line_span[line[ends - 1]] = np.arange(len(ends))
    skey = kn[ends]
    key_open = np.full(len(names), NONE, np.uint32)
    opens = np.flatnonzero(state == S_OPEN)
    key_open[kn[opens]] = line[opens]
    return {"span_key": skey.astype(np.uint32), "span_begin_line": line[ends - 1].astype(np.uint32), "span_end_line": line[ends].astype(np.uint32),
            "span_begin": tt[ends - 1].astype(np.int64), "span_end": tt[ends].astype(np.int64), "span_duration": (tt[ends] - tt[ends - 1]).astype(np.int64),
            "span_class": np.zeros(len(ends), np.uint8), "key_span_begin": np.searchsorted(skey, np.arange(len(names) + 1)).astype(np.uint64),
            "key_open_line": key_open, "line_span": line_span, "line_state": line_state}
