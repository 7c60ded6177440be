"""The rule of gx_group_lines restated in Python, for the tests of both sides (tests/test_group_host.py: the probing code of
gx_group.hpp as a program under sanitizers; tests/test_gpu_group.py: the kernels): a dict filled line by line, whose insertion order
is the order of the keys.  A line counts when its outcome is an extraction that has a part and every term of that extraction holds
(where_oracle.keep_lines); its key is sliced out of the line with the capture offsets (where_oracle.pair_set); the measured value is
parsed with where_oracle.parse_long and summed in Python's integers (stats_oracle.summarise)."""
import numpy as np

from stats_oracle import summarise
from where_oracle import keep_lines, outcome, pair_set, unpack

NONE = 0xFFFFFFFF


def decode_parts(p):
    """Gorp.group_parts' result as [(extraction, key group, value group or -1)]."""
    return [(p.array[t].extraction, p.array[t].key_group, p.array[t].value_group) for t in range(p.n)]


def group_values(values):
    """The dictionary encoding of a sequence of hashable values (None: no key): (keys in order of first appearance, first index per key,
    count per key, key number per value or NONE)."""
    number, first, count, line_key = {}, [], [], []
    for i, v in enumerate(values):
        if v is None:
            line_key.append(NONE)
            continue
        if v not in number:
            number[v] = len(first)
            first.append(i)
            count.append(0)
        count[number[v]] += 1
        line_key.append(number[v])
    return list(number), first, count, line_key


def group_lines(data, offsets, ids, caps, parts, terms, K):
    """What gx_group_lines delivers.  ids: int32 match ids and caps their dense rows, or ids = u16 / u8 result rows (caps None); parts:
    decode_parts'; terms: where_oracle.decode_terms'.  Returns a dict: keys (tuples of code units), first_line, lines, stats (None when
    no part has a value group), line_key, totals."""
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    by_k = {k: (g, v) for k, g, v in parts}
    counted = np.isin(oc, list(by_k))
    keep = np.zeros(len(oc), bool)
    if counted.any():
        keep[counted] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[counted] if terms else True

    def value(i, g):
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        return tuple(data[off[i] + b:off[i] + e].tolist()) if pair_set(b, e, off[i + 1] - off[i]) else None

    line_values = [value(i, by_k[int(oc[i])][0]) if keep[i] else None for i in range(len(oc))]
    keys, first, count, line_key = group_values(line_values)
    has_values = any(v >= 0 for _, _, v in parts)
    measured = [[] for _ in keys]
    for i in np.flatnonzero(keep):
        vg = by_k[int(oc[i])][1]
        if line_key[i] != NONE and vg >= 0:
            measured[line_key[i]].append(value(i, vg))
    stats = None
    if has_values:
        stats = [{k: v for k, v in summarise(m, []).items() if k != "hist"} for m in measured]
    lines = int(keep.sum())
    keyed = sum(1 for j in line_key if j != NONE)
    return {"keys": keys, "first_line": first, "lines": count, "stats": stats, "line_key": line_key,
            "totals": {"n_keys": len(keys), "key_units": sum(len(k) for k in keys), "lines": lines, "keyed": keyed, "unset": lines - keyed, "exact": True}}


def same(got, want, data_dtype=np.uint8):
    """Gorp.group_lines' dict (keys="csr" or "list") against group_lines': every field, bit for bit."""
    k = len(want["keys"])
    assert got["totals"] == want["totals"], (got["totals"], want["totals"])
    koff = np.asarray(got["key_offsets"]).astype(np.int64)
    units = np.asarray(got["key_units"])
    assert units.dtype == data_dtype and len(koff) == k + 1 and koff[0] == 0 and koff[-1] == len(units) == want["totals"]["key_units"]
    assert [tuple(units[koff[j]:koff[j + 1]].tolist()) for j in range(k)] == want["keys"]
    assert np.asarray(got["first_line"]).dtype == np.uint32 and np.asarray(got["first_line"]).tolist() == want["first_line"]
    assert np.asarray(got["lines"]).dtype == np.uint64 and np.asarray(got["lines"]).tolist() == want["lines"]
    assert np.asarray(got["line_key"]).dtype == np.uint32 and np.asarray(got["line_key"]).tolist() == want["line_key"]
    assert (got["stats"] is None) == (want["stats"] is None)
    if want["stats"] is not None:
        assert len(got["stats"]) == k
        for j, (g, w) in enumerate(zip(got["stats"], want["stats"])):
            assert g["lines"] == g["numbers"] + g["unset"] + g["not_numbers"], (j, g)
            assert g == w, (j, g, w)
    assert sorted(want["first_line"]) == want["first_line"] and sum(want["lines"]) == want["totals"]["keyed"]
    return True


# ---------------------------------------------------------------------------
# the table itself (gx_group.hpp), for the program under sanitizers
# ---------------------------------------------------------------------------
M64 = 2 ** 64 - 1


def hash_units(units, weak=False):
    """gx_group.hpp's group_hash: FNV-1a over the units, then the finishing mix; weak: the low 3 bits."""
    h = 0xCBF29CE484222325
    for u in units:
        h = ((h ^ u) * 0x100000001B3) & M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h & 7 if weak else h


def slots_for(max_keys):
    s = 64
    while s < 2 * max_keys:
        s *= 2
    return s


def probe_table(values, slots, weak=False):
    """Linear probing from hash & (slots - 1): per value its slot or None ("full"), and the table as {slot: (line, tag)}."""
    table, keys, out = {}, {}, []
    for i, v in enumerate(values):
        h = hash_units(v, weak)
        s, found = h & (slots - 1), None
        for _ in range(slots):
            if s not in table:
                table[s], keys[s] = (i, h >> 32), tuple(v)
                found = s
                break
            if keys[s] == tuple(v):
                found = s
                break
            s = (s + 1) & (slots - 1)
        out.append(found)
    return out, table
