"""The rule of gx_group_sessions restated in Python, for the tests of both sides (tests/test_sessions_host.py; tests/test_gpu_sessions.py:
the kernels), line by line: a line counts when its outcome is an extraction that has a part and every term of that extraction holds
(where_oracle.keep_lines); it is keyed when its key group names a value (where_oracle.pair_set); a keyed line's time is sliced out of the
line with the capture offsets and parsed under its format (number_oracle.parse); the entries are a dict of lists keyed by the key's
bytes, each list sorted by (time, line), and a loop with Python's integers cuts it wherever time - previous time > max_gap: nothing can
overflow.  The measured values are summed in Python's integers (bucket_oracle.summarise)."""
import numpy as np

from bucket_oracle import INT64_MAX, INT64_MIN, NONE, summarise
from number_oracle import LONG, parse
from series_oracle import batch, decode_parts, digits_batch
from where_oracle import keep_lines, outcome, pair_set, unpack

assert (INT64_MIN, INT64_MAX, NONE) == (-2 ** 63, 2 ** 63 - 1, 0xFFFFFFFF) and batch and decode_parts and digits_batch

SESSION_FIELDS = (("session_key", np.uint32), ("session_begin", np.int64), ("session_end", np.int64), ("session_first_line", np.uint32),
                  ("session_lines", np.uint64), ("session_entry_begin", np.uint64), ("key_session_begin", np.uint64), ("entry_line", np.uint32),
                  ("line_session", np.uint32))
SESSION_TOTALS = ("n_sessions", "entries", "number_unset", "not_numbers", "longest_lines", "longest_duration", "first_time", "last_time")


def opens(prev, t, max_gap):
    """the gap rule on Python's integers: prev <= t"""
    return t - prev > max_gap


def group_sessions(data, offsets, ids, caps, parts, max_gap, terms, K, formats=None):
    """What gx_group_sessions delivers beside gx_group_lines' outputs, and the group totals it rests on.  ids: int32 match ids and caps
    their dense rows, or ids = u16 / u8 result rows (caps None); parts: decode_parts' (extraction, key group, value group or -1, number
    group or -1); terms: where_oracle.decode_terms'; formats: {(extraction, group): (kind, scale)}, LONG where absent."""
    formats = formats or {}
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    by_k = {k: (kg, vg, ng) for k, kg, vg, ng in parts}
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
            return 1, None
        v = parse(*formats.get((int(oc[i]), g), (LONG, 0)), t.tolist())
        return (2, None) if v is None else (0, v)

    has_values = any(vg >= 0 for _, _, vg, _ in parts)
    key_number, by_key = {}, {}
    totals = {"lines": int(keep.sum()), "keyed": 0, "unset": 0, "entries": 0, "number_unset": 0, "not_numbers": 0}
    for i in range(len(oc)):
        if not keep[i]:
            continue
        kg, vg, ng = by_k[int(oc[i])]
        key = text(i, kg)
        if key is None:
            totals["unset"] += 1
            continue
        totals["keyed"] += 1
        key = (key.dtype.itemsize, key.tobytes())
        j = key_number.setdefault(key, len(key_number))
        cls, t = number(i, ng) if ng >= 0 else (1, None)
        if cls:
            totals["number_unset" if cls == 1 else "not_numbers"] += 1
            continue
        totals["entries"] += 1
        by_key.setdefault(j, []).append((t, i, number(i, vg) if vg >= 0 else None))
    sessions, entry_line = [], []
    line_session = [NONE] * len(oc)
    key_begin = []
    for j in range(len(key_number)):
        key_begin.append(len(sessions))
        prev = None
        for t, i, value in sorted(by_key.get(j, []), key=lambda e: (e[0], e[1])):
            if prev is None or opens(prev, t, max_gap):
                sessions.append({"key": j, "begin": t, "end": t, "first": i, "lines": 0, "at": len(entry_line), "numbers": [], "unset": 0, "nan": 0})
            s = sessions[-1]
            s["end"] = t
            s["lines"] += 1
            if value is not None:
                if value[0] == 0:
                    s["numbers"].append(value[1])
                else:
                    s["unset" if value[0] == 1 else "nan"] += 1
            line_session[i] = len(sessions) - 1
            entry_line.append(i)
            prev = t
    key_begin.append(len(sessions))
    times = [t for es in by_key.values() for t, _, _ in es]
    totals.update(n_keys=len(key_number), n_sessions=len(sessions), longest_lines=max([s["lines"] for s in sessions], default=0),
                  longest_duration=max([s["end"] - s["begin"] for s in sessions], default=0), first_time=min(times, default=0), last_time=max(times, default=0))
    assert totals["keyed"] == totals["entries"] + totals["number_unset"] + totals["not_numbers"]
    return {"session_key": [s["key"] for s in sessions], "session_begin": [s["begin"] for s in sessions], "session_end": [s["end"] for s in sessions],
            "session_first_line": [s["first"] for s in sessions], "session_lines": [s["lines"] for s in sessions],
            "session_stats": [summarise(s["numbers"], s["unset"], s["nan"]) for s in sessions] if has_values else None,
            "session_entry_begin": [s["at"] for s in sessions] + [len(entry_line)], "key_session_begin": key_begin, "entry_line": entry_line,
            "line_session": line_session, "totals": totals, "keys": [k[1] for k in key_number]}


def same(got, want):
    """Gorp.group_sessions' dict against group_sessions': every session field and total, bit for bit."""
    t, g = want["totals"], got["totals"]
    for name in t:
        assert g[name] == t[name], (name, g[name], t[name])
    for name, dtype in SESSION_FIELDS:
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    assert (got["session_stats"] is None) == (want["session_stats"] is None)
    if want["session_stats"] is not None:
        assert len(got["session_stats"]) == len(want["session_stats"])
        for j, (a, b) in enumerate(zip(got["session_stats"], want["session_stats"])):
            assert a == b, (j, a, b)
    assert sum(want["session_lines"]) == t["entries"] and want["key_session_begin"][-1] == t["n_sessions"]
    return True


# ---------------------------------------------------------------------------
# the large shape: key numbers and times as arrays, the batch written by numpy alone (digits_batch takes a one-letter key; here the key
# is a number in KEY_DIGITS digits), and the restatement by lexsort + diff in uint64
# ---------------------------------------------------------------------------
KEY_DIGITS, TIME_DIGITS = 5, 10


def draw(n, seed, n_keys=5000, span=3_000_000_000, none=0.03):
    """n (key, time) lines in no order at all, times with ties, and a share of lines that match nothing"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_keys, n).astype(np.int64), rng.integers(0, span, n).astype(np.int64) // 1000 * 1000, rng.random(n) >= none


def wide_batch(key, t, matched):
    """every line is its key in KEY_DIGITS decimal digits, its time in TIME_DIGITS, zero-padded, and one byte of filler"""
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
    return data.reshape(-1), offsets, np.where(matched, 0, -1).astype(np.int32), caps


def np_sessions(key, t, matched, max_gap):
    """{field: array}: key numbers by first appearance, np.lexsort by (key number, time, line), the gaps by np.diff in uint64"""
    n = len(t)
    at = np.flatnonzero(matched)
    names, first = np.unique(key[at], return_index=True)
    number_of = np.zeros(int(names.max()) + 1 if len(names) else 1, np.int64)
    number_of[names[np.argsort(first)]] = np.arange(len(names))
    kn = number_of[key[at]]
    order = np.lexsort((at, t[at], kn))
    kn, tt, line = kn[order], t[at][order], at[order]
    gap = np.diff(tt.astype(np.uint64))                                   # (wraps where the key changes: those are heads anyway)
    head = np.concatenate([[True], (np.diff(kn) != 0) | (gap > np.uint64(max_gap))]) if len(at) else np.zeros(0, bool)
    start = np.flatnonzero(head)
    end = np.concatenate([start[1:], [len(at)]]) if len(start) else start
    line_session = np.full(n, NONE, np.uint32)
    line_session[line] = (np.cumsum(head) - 1).astype(np.uint32)
    skey = kn[start]
    return {"session_key": skey.astype(np.uint32), "session_begin": tt[start].astype(np.int64), "session_end": tt[end - 1].astype(np.int64),
            "session_first_line": line[start].astype(np.uint32), "session_lines": (end - start).astype(np.uint64),
            "session_entry_begin": np.concatenate([start, [len(at)]]).astype(np.uint64),
            "key_session_begin": np.searchsorted(skey, np.arange(len(names) + 1)).astype(np.uint64), "entry_line": line.astype(np.uint32),
            "line_session": line_session}
