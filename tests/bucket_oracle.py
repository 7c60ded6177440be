"""The rule of gx_bucket_lines restated in Python, for the tests of both sides (tests/test_bucket_host.py: gx_bucket.hpp as a program
under sanitizers; tests/test_gpu_bucket.py: the kernels), line by line: a line counts when its outcome is an extraction that has a part
and every term of that extraction holds (where_oracle.keep_lines); its number is sliced out of the line with the capture offsets
(where_oracle.pair_set) and parsed under its format (number_oracle.parse); its bucket is Python's // on unbounded ints; the buckets are
a dict sorted by key; the measured values are summed in Python's integers (stats_oracle.summarise's fields)."""
import numpy as np

from number_oracle import LONG, parse
from where_oracle import keep_lines, outcome, pair_set, unpack

NONE = 0xFFFFFFFF
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
M64 = 2 ** 64 - 1


def bucket_of(v, origin, width):
    """floor((v - origin) / width), or None outside [INT64_MIN + 1, INT64_MAX]"""
    b = (v - origin) // width
    return b if INT64_MIN < b <= INT64_MAX else None


def decode_parts(p):
    """Gorp.bucket_parts' result as [(extraction, number group, value group or -1)]."""
    return [(p.array[t].extraction, p.array[t].number_group, p.array[t].value_group) for t in range(p.n)]


def summarise(numbers, unset, nan):
    return {"lines": len(numbers) + unset + nan, "numbers": len(numbers), "unset": unset, "not_numbers": nan, "min": min(numbers) if numbers else None,
            "max": max(numbers) if numbers else None, "sum": sum(numbers)}


def bucket_lines(data, offsets, ids, caps, parts, origin, width, terms, K, formats=None):
    """What gx_bucket_lines delivers.  ids: int32 match ids and caps their dense rows, or ids = u16 / u8 result rows (caps None); parts:
    decode_parts'; terms: where_oracle.decode_terms'; formats: {(extraction, group): (kind, scale)}, LONG where absent."""
    formats = formats or {}
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    by_k = {k: (g, v) for k, g, v in parts}
    counted = np.isin(oc, list(by_k))
    keep = np.zeros(len(oc), bool)
    if counted.any():
        keep[counted] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[counted] if terms else True

    def number(i, g):
        """(class, value): 0 a number, 1 unset, 2 no number"""
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        if not pair_set(b, e, off[i + 1] - off[i]):
            return 1, None
        v = parse(*formats.get((int(oc[i]), g), (LONG, 0)), data[off[i] + b:off[i] + e].tolist())
        return (2, None) if v is None else (0, v)

    has_values = any(v >= 0 for _, _, v in parts)
    buckets, line_b = {}, []
    totals = {"lines": int(keep.sum()), "bucketed": 0, "unset": 0, "not_numbers": 0, "out_of_range": 0}
    for i in range(len(oc)):
        line_b.append(None)
        if not keep[i]:
            continue
        g, vg = by_k[int(oc[i])]
        cls, v = number(i, g)
        if cls:
            totals["unset" if cls == 1 else "not_numbers"] += 1
            continue
        b = bucket_of(v, origin, width)
        if b is None:
            totals["out_of_range"] += 1
            continue
        totals["bucketed"] += 1
        line_b[i] = b
        row = buckets.setdefault(b, {"first": i, "lines": 0, "numbers": [], "unset": 0, "nan": 0})
        row["lines"] += 1
        if vg >= 0:
            cls, v = number(i, vg)
            if cls == 0:
                row["numbers"].append(v)
            else:
                row["unset" if cls == 1 else "nan"] += 1
    order = sorted(buckets)
    rank = {b: j for j, b in enumerate(order)}
    totals.update(n_buckets=len(order), exact=True, first_bucket=order[0] if order else 0, last_bucket=order[-1] if order else 0)
    return {"bucket_number": order, "first_line": [buckets[b]["first"] for b in order], "lines": [buckets[b]["lines"] for b in order],
            "stats": [summarise(buckets[b]["numbers"], buckets[b]["unset"], buckets[b]["nan"]) for b in order] if has_values else None,
            "line_bucket": [NONE if b is None else rank[b] for b in line_b], "totals": totals}


def same(got, want):
    """Gorp.bucket_lines' dict against bucket_lines': every field, bit for bit."""
    assert got["totals"] == want["totals"], (got["totals"], want["totals"])
    t = want["totals"]
    assert t["lines"] == t["bucketed"] + t["unset"] + t["not_numbers"] + t["out_of_range"]
    for name, dtype in (("bucket_number", np.int64), ("first_line", np.uint32), ("lines", np.uint64), ("line_bucket", np.uint32)):
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    assert (got["stats"] is None) == (want["stats"] is None)
    if want["stats"] is not None:
        assert len(got["stats"]) == len(want["stats"])
        for j, (g, w) in enumerate(zip(got["stats"], want["stats"])):
            assert g == w, (j, g, w)
    assert sorted(set(want["bucket_number"])) == want["bucket_number"] and sum(want["lines"]) == t["bucketed"]
    return True


def batch(numbers, values=None, lengths=None, ids=None, dtype=np.uint8, offsets_dtype=np.uint32, groups=2, filler=0x2E):
    """A line is its number's text, its value's text (ints, bytes or None: that group is unset) and filler up to lengths[i] units.
    Returns (data, offsets, ids, caps): group 0 is the number, group 1 the value, further groups unset."""
    text = lambda v: None if v is None else v if isinstance(v, bytes) else b"%d" % int(v)
    a = [text(v) for v in numbers]
    b = [None] * len(a) if values is None else [text(v) for v in values]
    n = len(a)
    alen = np.array([0 if k is None else len(k) for k in a], np.int64)
    blen = np.array([0 if s is None else len(s) for s in b], np.int64)
    lens = alen + blen if lengths is None else np.maximum(np.asarray(lengths, np.int64), alen + blen)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(offsets_dtype)
    data = np.full(int(lens.sum()), filler, dtype)
    caps = np.full((n, 2 * groups), -1, np.int32)
    for i in range(n):
        o = int(offsets[i])
        if a[i] is not None:
            data[o:o + alen[i]] = np.frombuffer(a[i], np.uint8)
            caps[i, 0], caps[i, 1] = 0, alen[i]
        if b[i] is not None:
            data[o + alen[i]:o + alen[i] + blen[i]] = np.frombuffer(b[i], np.uint8)
            caps[i, 2], caps[i, 3] = alen[i], alen[i] + blen[i]
    return data, offsets, np.zeros(n, np.int32) if ids is None else np.asarray(ids, np.int32), caps


# ---------------------------------------------------------------------------
# the large shape: numbers of a fixed width written by numpy alone, and the restatement by np.unique
# ---------------------------------------------------------------------------
DIGITS = 10


def draw(n, seed, span=5_000_000, none=0.03):
    """n numbers in [0, span) that mostly ascend (a time-ordered log with jitter) and a share of lines that match nothing"""
    rng = np.random.default_rng(seed)
    v = np.sort(rng.integers(0, span, n)) + rng.integers(-2000, 2000, n)
    v = np.clip(v, 0, 10 ** DIGITS - 1).astype(np.int64)
    matched = rng.random(n) >= none
    return v, matched


def digits_batch(v, matched):
    """every line is its number in DIGITS decimal digits, zero-padded, and one byte of filler"""
    n = len(v)
    data = np.full((n, DIGITS + 1), 0x2E, np.uint8)
    q = v.copy()
    for d in range(DIGITS - 1, -1, -1):
        data[:, d] = 48 + q % 10
        q //= 10
    offsets = (np.arange(n + 1, dtype=np.int64) * (DIGITS + 1)).astype(np.uint32)
    caps = np.tile(np.array([0, DIGITS, -1, -1], np.int32), (n, 1))
    return data.reshape(-1), offsets, np.where(matched, 0, -1).astype(np.int32), caps


def np_buckets(v, matched, origin, width):
    """(bucket_number int64, first_line uint32, lines uint64, line_bucket uint32) by np.unique on (v - origin) // width"""
    b = np.floor_divide(v - origin, width)
    at = np.flatnonzero(matched)
    number, first, inverse, count = np.unique(b[at], return_index=True, return_inverse=True, return_counts=True)
    line_bucket = np.full(len(v), NONE, np.uint32)
    line_bucket[at] = inverse.astype(np.uint32)
    return number.astype(np.int64), at[first].astype(np.uint32), count.astype(np.uint64), line_bucket


# ---------------------------------------------------------------------------
# the table itself (gx_bucket.hpp), for the program under sanitizers
# ---------------------------------------------------------------------------
def word_of(b):
    return (b & M64) ^ (1 << 63)


def bucket_hash(word, weak=False):
    """gx_bucket.hpp's bucket_hash: group_hash's finishing mix over the word; weak: the low 3 bits."""
    h = word
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h & 7 if weak else h


def probe_words(words, slots, weak=False):
    """Linear probing from hash & (slots - 1): per word its slot or None ("full"), and the table as {slot: word}."""
    table, out = {}, []
    for w in words:
        s, found = bucket_hash(w, weak) & (slots - 1), None
        for _ in range(slots):
            if s not in table:
                table[s] = w
            if table[s] == w:
                found = s
                break
            s = (s + 1) & (slots - 1)
        out.append(found)
    return out, table


def digits_of(min_word, max_word):
    return ((min_word ^ max_word).bit_length() + 5) // 6
