"""The rule of gx_group_windows restated in Python, for the tests of both sides (tests/test_windows_host.py; tests/test_gpu_windows.py: the
kernels), line by line.  Lines count, are keyed and are entries exactly as in sessions_oracle.group_sessions; per key the entries are
sorted by (time, line) and the caller's own loop runs over them with Python's integers, so nothing can wrap:
    q.addLast(t);  while (t - q.peekFirst() > window) q.removeFirst();
The deque's size is window_lines; a trip is the entry at which it reaches the threshold from below; the window's sum is over the deque's
values that are numbers."""
from collections import deque

import numpy as np

from number_oracle import LONG, parse
from sessions_oracle import INT64_MAX, INT64_MIN, NONE, batch, decode_parts, draw, wide_batch
from where_oracle import keep_lines, outcome, pair_set, unpack

assert (INT64_MIN, INT64_MAX, NONE) == (-2 ** 63, 2 ** 63 - 1, 0xFFFFFFFF) and batch and decode_parts and draw and wide_batch

WINDOW_FIELDS = (("entry_line", np.uint32), ("entry_key", np.uint32), ("entry_time", np.int64), ("entry_window_lines", np.uint32),
                 ("key_entry_begin", np.uint64), ("key_peak_lines", np.uint32), ("key_peak_line", np.uint32), ("line_window_lines", np.uint32),
                 ("trip_key", np.uint32), ("trip_line", np.uint32), ("trip_time", np.int64), ("trip_entry", np.uint32), ("key_trip_begin", np.uint64))
WINDOW_TOTALS = ("entries", "number_unset", "not_numbers", "n_trips", "tripped_keys", "peak_lines", "peak_line", "peak_key", "first_time", "last_time")


def holds(f_time, e_time, window):
    """the window's predicate on Python's integers: f_time <= e_time"""
    return e_time - f_time <= window


def key_windows(entries, window, threshold):
    """One key's entries [(time, line, value or None)], sorted by (time, line), through the deque: per entry (window_lines, trips,
    numbers in the window, their sum)."""
    q, out, prev = deque(), [], None
    for t, i, value in entries:
        q.append((t, value))
        while not holds(q[0][0], t, window):
            q.popleft()
        lines = len(q)
        trips = threshold != 0 and lines >= threshold and (prev is None or prev < threshold)
        numbers = [v[1] for _, v in q if v is not None and v[0] == 0]
        out.append((lines, trips, len(numbers), sum(numbers)))
        prev = lines
    return out


def group_windows(data, offsets, ids, caps, parts, window, threshold, terms, K, formats=None):
    """What gx_group_windows delivers beside gx_group_lines' outputs, and the group totals it rests on.  Arguments as
    sessions_oracle.group_sessions takes them."""
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
    res = {name: [] for name, _ in WINDOW_FIELDS}
    res["entry_window_sum"] = [] if has_values else None
    res["line_window_lines"] = [0] * len(oc)
    tripped = 0
    peak = (0, NONE, NONE)
    for j in range(len(key_number)):
        res["key_entry_begin"].append(len(res["entry_line"]))
        res["key_trip_begin"].append(len(res["trip_key"]))
        entries = sorted(by_key.get(j, []), key=lambda e: (e[0], e[1]))
        kpeak, kline, first = 0, NONE, True
        for (t, i, _), (lines, trips, numbers, total) in zip(entries, key_windows(entries, window, threshold)):
            e = len(res["entry_line"])
            res["entry_line"].append(i)
            res["entry_key"].append(j)
            res["entry_time"].append(t)
            res["entry_window_lines"].append(lines)
            res["line_window_lines"][i] = lines
            if has_values:
                res["entry_window_sum"].append({"numbers": numbers, "sum": total})
            if trips:
                res["trip_key"].append(j)
                res["trip_line"].append(i)
                res["trip_time"].append(t)
                res["trip_entry"].append(e)
                tripped += first
                first = False
            if lines > kpeak:
                kpeak, kline = lines, i
            if lines > peak[0]:
                peak = (lines, i, j)
        res["key_peak_lines"].append(kpeak)
        res["key_peak_line"].append(kline)
    res["key_entry_begin"].append(len(res["entry_line"]))
    res["key_trip_begin"].append(len(res["trip_key"]))
    times = res["entry_time"]
    totals.update(n_keys=len(key_number), n_trips=len(res["trip_key"]), tripped_keys=tripped, peak_lines=peak[0], peak_line=peak[1], peak_key=peak[2],
                  first_time=min(times, default=0), last_time=max(times, default=0))
    assert totals["keyed"] == totals["entries"] + totals["number_unset"] + totals["not_numbers"]
    res.update(totals=totals, keys=[k[1] for k in key_number])
    return res


def same(got, want):
    """Gorp.group_windows' dict against group_windows': every window field and total, bit for bit."""
    t, g = want["totals"], got["totals"]
    for name in t:
        assert g[name] == t[name], (name, g[name], t[name])
    for name, dtype in WINDOW_FIELDS:
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    assert (got["entry_window_sum"] is None) == (want["entry_window_sum"] is None)
    if want["entry_window_sum"] is not None:
        assert len(got["entry_window_sum"]) == len(want["entry_window_sum"])
        for e, (a, b) in enumerate(zip(got["entry_window_sum"], want["entry_window_sum"])):
            assert a == b, (e, a, b)
    assert len(want["entry_line"]) == t["entries"] and want["key_trip_begin"][-1] == t["n_trips"]
    return True


# ---------------------------------------------------------------------------
# the large shape (sessions_oracle.draw / wide_batch): key numbers by first appearance, np.lexsort by (key number, time, line), and per
# key np.searchsorted on the order-preserving words with a saturating word - window
# ---------------------------------------------------------------------------
def np_windows(key, t, matched, window, threshold):
    """{field: array} and the totals' trips and peak"""
    n = len(t)
    at = np.flatnonzero(matched)
    m = len(at)
    names, first = np.unique(key[at], return_index=True)
    number_of = np.zeros(int(names.max()) + 1 if len(names) else 1, np.int64)
    number_of[names[np.argsort(first)]] = np.arange(len(names))
    kn = number_of[key[at]]
    order = np.lexsort((at, t[at], kn))
    kn, tt, line = kn[order], t[at][order], at[order]
    word = tt.astype(np.uint64) ^ np.uint64(1 << 63)                              # order-preserving: the time with its sign bit flipped
    w = np.uint64(window)
    floor = np.where(word >= w, word - np.minimum(word, w), np.uint64(0))         # saturating word - window
    begin = np.searchsorted(kn, np.arange(len(names) + 1))
    lo = np.zeros(m, np.int64)
    for j in range(len(names)):
        b, e = int(begin[j]), int(begin[j + 1])
        lo[b:e] = b + np.searchsorted(word[b:e], floor[b:e], side="left")
    wl = (np.arange(m) - lo + 1).astype(np.uint32)
    head = np.concatenate([[True], np.diff(kn) != 0]) if m else np.zeros(0, bool)
    prev = np.concatenate([[0], wl[:-1]]) if m else wl
    trip = (wl >= threshold) & (head | (prev < threshold)) if threshold else np.zeros(m, bool)
    te = np.flatnonzero(trip)
    line_wl = np.zeros(n, np.uint32)
    line_wl[line] = wl
    kpl, kpline = np.zeros(len(names), np.uint32), np.full(len(names), NONE, np.uint32)
    for j in range(len(names)):
        b, e = int(begin[j]), int(begin[j + 1])
        if e > b:
            p = b + int(np.argmax(wl[b:e]))                                      # (argmax: the first that attains the maximum)
            kpl[j], kpline[j] = wl[p], line[p]
    p = int(np.argmax(wl)) if m else -1
    return {"entry_line": line.astype(np.uint32), "entry_key": kn.astype(np.uint32), "entry_time": tt.astype(np.int64), "entry_window_lines": wl,
            "key_entry_begin": begin.astype(np.uint64), "key_peak_lines": kpl, "key_peak_line": kpline, "line_window_lines": line_wl,
            "trip_key": kn[te].astype(np.uint32), "trip_line": line[te].astype(np.uint32), "trip_time": tt[te].astype(np.int64), "trip_entry": te.astype(np.uint32),
            "key_trip_begin": np.searchsorted(kn[te], np.arange(len(names) + 1)).astype(np.uint64),
            "totals": {"n_trips": len(te), "tripped_keys": len(np.unique(kn[te])), "peak_lines": int(wl[p]) if m else 0,
                       "peak_line": int(line[p]) if m else NONE, "peak_key": int(kn[p]) if m else NONE}}
