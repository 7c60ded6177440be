"""The rule of gx_capture_stats restated in Python, for the tests of both sides (tests/test_stats_host.py: the C++ rule as a program
under sanitizers; tests/test_gpu_stats.py: the kernel).  A line counts for a measure when its outcome is the measure's extraction and
every term of that extraction holds (where_oracle.keep_lines with every outcome wanted); its value is sliced out of the line with the
capture offsets (where_oracle.pair_set), parsed with where_oracle.parse_long, and summed in Python's integers, which never wrap."""
import bisect

import numpy as np

from where_oracle import INT64_MAX, INT64_MIN, keep_lines, outcome, pair_set, parse_long, unpack

# the three sequences whose sums leave int64: upwards, downwards, and mixed signs so that hi is negative while lo carries
SUM_SEQUENCES = {
    "up": [(70000, INT64_MAX)],
    "down": [(70000, INT64_MIN)],
    "mixed": [(30000, -1), (20000, 0xFFFFFFFF), (10000, INT64_MIN + 0xFFFFFFFF), (5000, -0x100000001), (4999, 0x1FFFFFFFF), (1, INT64_MAX)],
}


def bucket(edges, v):
    """the number of edges <= v"""
    return bisect.bisect_right(list(edges), v)


def split128(total):
    """(sum_hi signed, sum_lo unsigned) of a Python int as a 128-bit two's-complement integer"""
    assert -2 ** 127 <= total < 2 ** 127
    return total >> 64, total & (2 ** 64 - 1)


def summarise(values, edges):
    """One measure's dict from its lines' values: None (unset) or sequences of code units."""
    edges = [int(e) for e in edges]
    hist = [0] * (len(edges) + 1)
    numbers, unset, nan = [], 0, 0
    for value in values:
        if value is None:
            unset += 1
            continue
        v = parse_long(list(value))
        if v is None:
            nan += 1
        else:
            numbers.append(v)
            hist[bucket(edges, v)] += 1
    return {"lines": len(numbers) + unset + nan, "numbers": len(numbers), "unset": unset, "not_numbers": nan, "min": min(numbers) if numbers else None,
            "max": max(numbers) if numbers else None, "sum": sum(numbers), "hist": hist}


def decode_measures(m):
    """Gorp.measures' result as [(extraction, group, edges)]."""
    return [(m.array[t].extraction, m.array[t].group, m.edges[t].tolist()) for t in range(m.n)]


def capture_stats(data, offsets, ids, caps, measures, terms, K):
    """What gx_capture_stats returns.  ids: int32 match ids and caps their dense rows, or ids = u16 / u8 result rows (caps None);
    measures: decode_measures'; terms: where_oracle.decode_terms'."""
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    measured = np.isin(oc, [k for k, _, _ in measures])
    keep = np.zeros(len(oc), bool)
    if measured.any():
        sub = np.flatnonzero(measured)
        if terms:
            # (keep_lines looks at whole batches: hand it the measured lines alone, each with its own offsets)
            keep[sub] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[sub]
        else:
            keep[sub] = True
    out = []
    for k, g, edges in measures:
        values = []
        for i in np.flatnonzero(keep & (oc == k)):
            b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
            values.append(data[off[i] + b:off[i] + e].tolist() if pair_set(b, e, off[i + 1] - off[i]) else None)
        out.append(summarise(values, edges))
    return out


def same(got, want):
    """Gorp.capture_stats' list against capture_stats': every field, bit for bit."""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g["lines"] == g["numbers"] + g["unset"] + g["not_numbers"], (t, g)
        assert int(np.sum(g["hist"], dtype=np.uint64)) == g["numbers"], (t, g)
        for key in ("lines", "numbers", "unset", "not_numbers", "min", "max", "sum"):
            assert g[key] == w[key], (t, key, g, w)
        assert np.asarray(g["hist"]).dtype == np.uint64 and np.asarray(g["hist"]).tolist() == list(w["hist"]), (t, g, w)
    return True
