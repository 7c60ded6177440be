"""The rule of gx_top_lines restated in Python, for the tests of both sides (tests/test_top_host.py: the C++ rule as a program under
sanitizers; tests/test_gpu_top.py: the kernels).  Every line is classed as tests/stats_oracle.py classes one -- it counts when its
outcome is an extraction that has a part and every term of that extraction holds; its value is unset, no number or a number -- and the
numbers are ranked with sorted(cands, key=(-v, line))[:N] (or (v, line) for the smallest)."""
import numpy as np

from where_oracle import keep_lines, outcome, pair_set, parse_long, unpack


def rank(cands, n, largest=True):
    """cands: [(value, line)].  The n first of them by (value descending -- or ascending --, line ascending)."""
    return sorted(cands, key=(lambda c: (-c[0], c[1])) if largest else (lambda c: (c[0], c[1])))[:n]


def totals_of(cands, top, unset, nan, units_top):
    last = top[-1][0] if top else 0
    return {"lines": len(cands) + unset + nan, "numbers": len(cands), "unset": unset, "not_numbers": nan, "n_top": len(top), "units_top": units_top,
            "last_value": last, "ties_left": (sum(1 for v, _ in cands if v == last) - sum(1 for v, _ in top if v == last)) if top else 0}


def decode_parts(p):
    """Gorp.top_parts' result as [(extraction, group)]."""
    return [(p.array[t].extraction, p.array[t].value_group) for t in range(p.n)]


def top_lines(data, offsets, ids, caps, parts, terms, K, n, largest=True):
    """What Gorp.top_lines returns but ids2 / rows2: (index, values, units, offsets, totals).  ids: int32 match ids and caps their dense
    rows, or ids = u16 / u8 result rows (caps None); parts: decode_parts'; terms: where_oracle.decode_terms'."""
    data = np.asarray(data)
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    group_of = dict(parts)
    ranked = np.isin(oc, list(group_of))
    keep = np.zeros(len(oc), bool)
    if ranked.any():
        sub = np.flatnonzero(ranked)
        keep[sub] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[sub] if terms else True
    cands, unset, nan = [], 0, 0
    for i in np.flatnonzero(keep):
        g = group_of[int(oc[i])]
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        if not pair_set(b, e, off[i + 1] - off[i]):
            unset += 1
            continue
        v = parse_long(data[off[i] + b:off[i] + e].tolist())
        if v is None:
            nan += 1
        else:
            cands.append((v, int(i)))
    top = rank(cands, n, largest)
    index = np.array([i for _, i in top], np.uint32)
    values = np.array([v for v, _ in top], np.int64)
    lens = np.array([off[i + 1] - off[i] for _, i in top], np.int64)
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.asarray(offsets).dtype)
    units = np.concatenate([data[off[i]:off[i + 1]] for _, i in top]) if top else np.zeros(0, data.dtype)
    return index, values, units, out_off, totals_of(cands, top, unset, nan, int(lens.sum()))
