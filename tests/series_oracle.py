"""The rule of gx_group_series restated in Python, for the tests of both sides (tests/test_series_host.py: gx_series.hpp as a program
under sanitizers; tests/test_gpu_series.py: the kernels), line by line: a line counts when its outcome is an extraction that has a part
and every term of that extraction holds (where_oracle.keep_lines); it is keyed when its key group names a value (where_oracle.pair_set);
a keyed line's number is sliced out of the line with the capture offsets and parsed under its format (number_oracle.parse); its bucket
is bucket_oracle.bucket_of; the cells are a dict keyed by (key bytes, bucket), ordered by (the key's first line, bucket); the measured
values are summed in Python's integers."""
import numpy as np

from bucket_oracle import INT64_MAX, INT64_MIN, M64, NONE, bucket_hash, bucket_of, digits_of, summarise
from number_oracle import LONG, parse
from where_oracle import keep_lines, outcome, pair_set, unpack

SERIES_FIELDS = (("bucket_number", np.int64), ("cell_key", np.uint32), ("cell_bucket", np.uint32), ("cell_first_line", np.uint32), ("cell_lines", np.uint64),
                 ("key_cell_begin", np.uint64), ("line_cell", np.uint32))
SERIES_TOTALS = ("n_cells", "n_buckets", "celled", "number_unset", "not_numbers", "out_of_range", "cells_exact", "first_bucket", "last_bucket")


def decode_parts(both):
    """Gorp.series_parts' result as [(extraction, key group, value group or -1, number group or -1)]."""
    p, numbers = both
    return [(p.array[t].extraction, p.array[t].key_group, p.array[t].value_group, numbers[t]) for t in range(p.n)]


def group_series(data, offsets, ids, caps, parts, origin, width, terms, K, formats=None):
    """What gx_group_series delivers beside gx_group_lines' outputs, and the group totals it rests on.  ids: int32 match ids and caps their
    dense rows, or ids = u16 / u8 result rows (caps None); parts: decode_parts'; terms: where_oracle.decode_terms'; formats: {(extraction,
    group): (kind, scale)}, LONG where absent."""
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
    key_number, cells, line_c = {}, {}, []
    totals = {"lines": int(keep.sum()), "keyed": 0, "unset": 0, "celled": 0, "number_unset": 0, "not_numbers": 0, "out_of_range": 0}
    for i in range(len(oc)):
        line_c.append(None)
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
        cls, v = number(i, ng) if ng >= 0 else (1, None)
        if cls:
            totals["number_unset" if cls == 1 else "not_numbers"] += 1
            continue
        b = bucket_of(v, origin, width)
        if b is None:
            totals["out_of_range"] += 1
            continue
        totals["celled"] += 1
        line_c[i] = (j, b)
        row = cells.setdefault((j, b), {"first": i, "lines": 0, "numbers": [], "unset": 0, "nan": 0})
        row["lines"] += 1
        if vg >= 0:
            cls, v = number(i, vg)
            if cls == 0:
                row["numbers"].append(v)
            else:
                row["unset" if cls == 1 else "nan"] += 1
    axis = sorted({b for _, b in cells})
    rank = {b: r for r, b in enumerate(axis)}
    order = sorted(cells)                                 # (key number = the key's first appearance, bucket)
    cell_of = {c: q for q, c in enumerate(order)}
    n_keys = len(key_number)
    begin = np.searchsorted(np.array([j for j, _ in order], np.int64), np.arange(n_keys + 1)).tolist()   # (a key without a cell: an empty run)
    totals.update(n_keys=n_keys, n_cells=len(order), n_buckets=len(axis), cells_exact=True, first_bucket=axis[0] if axis else 0, last_bucket=axis[-1] if axis else 0)
    assert totals["keyed"] == totals["celled"] + totals["number_unset"] + totals["not_numbers"] + totals["out_of_range"]
    return {"bucket_number": axis, "cell_key": [j for j, _ in order], "cell_bucket": [rank[b] for _, b in order], "cell_first_line": [cells[c]["first"] for c in order],
            "cell_lines": [cells[c]["lines"] for c in order],
            "cell_stats": [summarise(cells[c]["numbers"], cells[c]["unset"], cells[c]["nan"]) for c in order] if has_values else None,
            "key_cell_begin": begin, "line_cell": [NONE if c is None else cell_of[c] for c in line_c], "totals": totals, "keys": [k[1] for k in key_number]}


def same(got, want):
    """Gorp.group_series' dict against group_series': every series field and total, bit for bit."""
    t, g = want["totals"], got["totals"]
    for name in t:
        assert g[name] == t[name], (name, g[name], t[name])
    for name, dtype in SERIES_FIELDS:
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    assert (got["cell_stats"] is None) == (want["cell_stats"] is None)
    if want["cell_stats"] is not None:
        assert len(got["cell_stats"]) == len(want["cell_stats"])
        for j, (a, b) in enumerate(zip(got["cell_stats"], want["cell_stats"])):
            assert a == b, (j, a, b)
    assert sum(want["cell_lines"]) == t["celled"] and want["key_cell_begin"][-1] == t["n_cells"]
    return True


def batch(keys, numbers, values=None, lengths=None, ids=None, dtype=np.uint8, offsets_dtype=np.uint32, groups=3, filler=0x2E):
    """A line is its key's text, its number's text, its value's text (bytes, ints, or None: that group is unset) and filler up to
    lengths[i] units.  Returns (data, offsets, ids, caps): group 0 is the key, group 1 the number, group 2 the value."""
    text = lambda v: None if v is None else bytes(v) if isinstance(v, (bytes, bytearray)) else b"%d" % int(v)
    n = len(keys)
    cols = [[text(v) for v in keys], [text(v) for v in numbers], [None] * n if values is None else [text(v) for v in values]]
    lens = np.array([[0 if t is None else len(t) for t in col] for col in cols], np.int64).reshape(3, n)
    total = lens.sum(axis=0)
    if lengths is not None:
        total = np.maximum(np.asarray(lengths, np.int64), total)
    offsets = np.concatenate([[0], np.cumsum(total)]).astype(offsets_dtype)
    data = np.full(int(total.sum()), filler, dtype)
    caps = np.full((n, 2 * groups), -1, np.int32)
    for i in range(n):
        at = 0
        for g in range(3):
            t = cols[g][i]
            if t is None:
                continue
            o = int(offsets[i]) + at
            data[o:o + len(t)] = np.frombuffer(t, np.uint8)
            caps[i, 2 * g], caps[i, 2 * g + 1] = at, at + len(t)
            at += len(t)
    return data, offsets, np.zeros(n, np.int32) if ids is None else np.asarray(ids, np.int32), caps


# ---------------------------------------------------------------------------
# the large shape: a one-byte key and a number of a fixed width written by numpy alone, and the restatement by np.unique
# ---------------------------------------------------------------------------
DIGITS = 10


def draw(n, seed, n_keys=6, span=20_000_000, none=0.03):
    """n (key, number) lines whose numbers mostly ascend (a time-ordered log with jitter), and a share of lines that match nothing"""
    rng = np.random.default_rng(seed)
    v = np.sort(rng.integers(0, span, n)) + rng.integers(-2000, 2000, n)
    v = np.clip(v, 0, 10 ** DIGITS - 1).astype(np.int64)
    return rng.integers(0, n_keys, n).astype(np.int64), v, rng.random(n) >= none


def digits_batch(key, v, matched):
    """every line is its key as one letter, its number in DIGITS decimal digits, zero-padded, and one byte of filler"""
    n = len(v)
    data = np.full((n, DIGITS + 2), 0x2E, np.uint8)
    data[:, 0] = 65 + key
    q = v.copy()
    for d in range(DIGITS, 0, -1):
        data[:, d] = 48 + q % 10
        q //= 10
    offsets = (np.arange(n + 1, dtype=np.int64) * (DIGITS + 2)).astype(np.uint32)
    caps = np.tile(np.array([0, 1, 1, DIGITS + 1, -1, -1], np.int32), (n, 1))
    return data.reshape(-1), offsets, np.where(matched, 0, -1).astype(np.int32), caps


def np_series(key, v, matched, origin, width):
    """{field: array} by np.unique over (line_key, bucket): key numbers by first appearance, cells by (key number, bucket)"""
    n = len(v)
    at = np.flatnonzero(matched)
    b = np.floor_divide(v - origin, width)[at]
    letters, first = np.unique(key[at], return_index=True)
    number_of = np.zeros(int(letters.max()) + 1 if len(letters) else 1, np.int64)
    number_of[letters[np.argsort(first)]] = np.arange(len(letters))
    kn = number_of[key[at]]
    axis, brank = np.unique(b, return_inverse=True)
    word = kn * max(1, len(axis)) + brank
    cells, cfirst, inverse, count = np.unique(word, return_index=True, return_inverse=True, return_counts=True)
    line_cell = np.full(n, NONE, np.uint32)
    line_cell[at] = inverse.astype(np.uint32)
    cell_key = cells // max(1, len(axis))
    return {"bucket_number": axis.astype(np.int64), "cell_key": cell_key.astype(np.uint32), "cell_bucket": (cells % max(1, len(axis))).astype(np.uint32),
            "cell_first_line": at[cfirst].astype(np.uint32), "cell_lines": count.astype(np.uint64),
            "key_cell_begin": np.searchsorted(cell_key, np.arange(len(letters) + 1)).astype(np.uint64), "line_cell": line_cell}


# ---------------------------------------------------------------------------
# the words themselves (gx_series.hpp), for the program under sanitizers
# ---------------------------------------------------------------------------
def cell_word(kslot, bslot):
    return ((kslot << 32) | bslot) + 1


def cell_kslot(word):
    return (word - 1) >> 32


def cell_bslot(word):
    return (word - 1) & 0xFFFFFFFF


def sort_word(key_number, bucket_rank, n_buckets):
    return key_number * n_buckets + bucket_rank


def series_digits(n_keys, n_buckets):
    words = n_keys * n_buckets
    return digits_of(0, words - 1) if words else 0
