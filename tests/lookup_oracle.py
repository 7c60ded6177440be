"""The rule of gx_lookup_lines restated in Python, for the tests of both sides (tests/test_lookup_host.py; tests/test_gpu_lookup.py: the
kernels): the dictionary is a dict filled with setdefault(entry, j) for ascending j, so the lowest entry number stands for every
duplicate; the lines are read by group_oracle.py's loop -- a line counts when its outcome is an extraction that has a part and every term
of that extraction holds (where_oracle.keep_lines), its key is sliced out of the line with the capture offsets (where_oracle.pair_set),
the measured value is parsed with where_oracle.parse_long and summed in Python's integers (stats_oracle.summarise).  group_hash is
restated too (group_oracle.hash_units), for the tests that choose texts by the slot their probe starts in."""
import numpy as np

from group_oracle import hash_units, slots_for
from stats_oracle import summarise
from where_oracle import keep_lines, outcome, pair_set, unpack

NONE = 0xFFFFFFFF
MISS = 0xFFFFFFFE
KEEP_NOTHING, KEEP_HITS, KEEP_OTHERS = 0, 1, 2


def csr_entries(units, offsets):
    """The entries of a CSR dictionary as tuples of code units."""
    off = np.asarray(offsets).astype(np.int64)
    units = np.asarray(units)
    return [tuple(units[off[j]:off[j + 1]].tolist()) for j in range(len(off) - 1)]


def first_slot(units, m, weak=False):
    """The slot at which the probe for `units` starts in the table of a dictionary of m entries."""
    return hash_units(units, weak) & (slots_for(m) - 1)


def tag(units, weak=False):
    return hash_units(units, weak) >> 32


def lookup_lines(data, offsets, ids, caps, parts, terms, K, entries, keep=KEEP_NOTHING):
    """What gx_lookup_lines delivers.  ids: int32 match ids and caps their dense rows, or ids = u16 / u8 result rows (caps None); parts:
    group_oracle.decode_parts'; terms: where_oracle.decode_terms'; entries: tuples of code units.  Returns a dict: line_entry, entry_same,
    entry_lines, entry_first_line, entry_stats (None when no part has a value group), kept (the kept lines' numbers), totals."""
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    by_k = {k: (g, v) for k, g, v in parts}
    counted = np.isin(oc, list(by_k)) if by_k else np.zeros(len(oc), bool)
    counts = np.zeros(len(oc), bool)
    if counted.any():
        counts[counted] = keep_lines(data, off, ids, caps, np.ones(2 * K + 1, np.uint8), terms, K)[counted] if terms else True

    index = {}
    for j, e in enumerate(entries):
        index.setdefault(tuple(e), j)
    m = len(entries)
    entry_same = [index[tuple(e)] for e in entries]

    def value(i, g):
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        return tuple(data[off[i] + b:off[i] + e].tolist()) if pair_set(b, e, off[i + 1] - off[i]) else None

    line_entry, kept = [], []
    entry_lines, entry_first = [0] * m, [NONE] * m
    measured = [[] for _ in range(m)]
    has_values = any(v >= 0 for _, _, v in parts)
    lines = unset = hits = misses = 0
    for i in range(len(oc)):
        if not counts[i]:
            line_entry.append(NONE)
            continue
        lines += 1
        kg, vg = by_k[int(oc[i])]
        key = value(i, kg)
        if key is None:
            unset += 1
            line_entry.append(NONE)
            hit = False
        elif key in index:
            j = index[key]
            hits += 1
            line_entry.append(j)
            entry_lines[j] += 1
            if entry_first[j] == NONE:
                entry_first[j] = i
            if vg >= 0:
                measured[j].append(value(i, vg))
            hit = True
        else:
            misses += 1
            line_entry.append(MISS)
            hit = False
        if (keep == KEEP_HITS and hit) or (keep == KEEP_OTHERS and not hit):
            kept.append(i)
    stats = None
    if has_values:
        stats = [{k: v for k, v in summarise(mm, []).items() if k != "hist"} for mm in measured]
    units_out = int(sum(off[i + 1] - off[i] for i in kept))
    return {"line_entry": line_entry, "entry_same": entry_same, "entry_lines": entry_lines, "entry_first_line": entry_first, "entry_stats": stats, "kept": kept,
            "totals": {"entries": m, "distinct_entries": len(index), "hit_entries": sum(1 for c in entry_lines if c), "lines": lines, "keyed": lines - unset,
                       "unset": unset, "hits": hits, "misses": misses, "lines_out": len(kept), "units_out": units_out}}


def same(got, want):
    """Gorp.lookup_lines' dict against lookup_lines': every field, bit for bit (the kept batch is compared by the caller)."""
    assert got["totals"] == want["totals"], (got["totals"], want["totals"])
    t = want["totals"]
    assert t["lines"] == t["keyed"] + t["unset"] and t["keyed"] == t["hits"] + t["misses"]
    for f, dt in (("line_entry", np.uint32), ("entry_same", np.uint32), ("entry_lines", np.uint64), ("entry_first_line", np.uint32)):
        a = np.asarray(got[f])
        assert a.dtype == dt and a.tolist() == want[f], (f, a.tolist()[:20], want[f][:20])
    assert (got["entry_stats"] is None) == (want["entry_stats"] is None)
    if want["entry_stats"] is not None:
        assert len(got["entry_stats"]) == t["entries"]
        for j, (g, w) in enumerate(zip(got["entry_stats"], want["entry_stats"])):
            assert g["lines"] == g["numbers"] + g["unset"] + g["not_numbers"], (j, g)
            assert g == w, (j, g, w)
    if "index" in got:
        assert np.asarray(got["index"]).dtype == np.uint32 and np.asarray(got["index"]).tolist() == want["kept"]
    return True
