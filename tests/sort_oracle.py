"""The rule of gx_sort_lines restated in Python, for the tests of both sides (tests/test_sort_host.py: the class rule, the places and the
digit plan of gx_sort.hpp as a program under sanitizers; tests/test_gpu_sort.py: the kernels).  Every line is classed as
tests/top_oracle.py classes one -- it counts when its outcome is an extraction that has a part and every term of that extraction holds;
its value is unset, no number or a number (number_oracle.parse under the group's format, Long.parseLong without one) -- and then:
    STAMPED  its value is a number;
    CARRIED  (carry only) not stamped, and some earlier line is: it takes the value of the nearest earlier stamped line;
    REST     everything else.
The entries (stamped and carried) leave by sorted(entries, key=(value -- negated for descending --, line)), the rest lines behind them
in input order or not at all.  np_sort is the numpy restatement for the large case -- a forward fill and a stable argsort -- which
test_sort_host.py compares with the oracle on small draws."""
import numpy as np

import number_oracle as NO
from where_oracle import keep_lines, outcome, pair_set, parse_long, unpack

STAMPED, CARRIED, REST = 0, 1, 2
DIGITS, DIGIT_BITS = 11, 6


def decode_parts(p):
    """Gorp.top_parts' result as [(extraction, group)]."""
    return [(p.array[t].extraction, p.array[t].value_group) for t in range(p.n)]


def key_of(value, descending=False):
    """gx_top.hpp's top_key(value, descending): order-preserving int64 -> uint64, complemented for descending"""
    k = (value + 2 ** 63) & (2 ** 64 - 1)
    return k ^ (2 ** 64 - 1) if descending else k


def plan(keys, all_digits=False):
    """the six-bit digits (from the least significant) in which two of the keys differ; all eleven with all_digits (and a key)"""
    if not keys:
        return []
    differ = 0
    for k in keys:
        differ |= k ^ keys[0]
    return [d for d in range(DIGITS) if all_digits or (differ >> (DIGIT_BITS * d)) & 63]


def classes(stamped, carry):
    """per line: STAMPED / CARRIED / REST, from the per-line `stamped` flags"""
    out, seen = [], False
    for s in stamped:
        seen = seen or bool(s)
        out.append(STAMPED if s else CARRIED if carry and seen else REST)
    return out


def order_of(values, carry=False, descending=False, rest_last=False):
    """values: per line an int (stamped) or None.  (index, out_values, out_class, carried, rest): the entries by (value, line) -- the
    value negated for descending --, the rest lines behind them in input order with rest_last."""
    cls = classes([v is not None for v in values], carry)
    entries, last = [], None
    for i, v in enumerate(values):
        last = v if v is not None else last
        if cls[i] != REST:
            entries.append((last, i))
    entries = sorted(entries, key=(lambda e: (-e[0], e[1])) if descending else (lambda e: (e[0], e[1])))
    rest = [i for i, c in enumerate(cls) if c == REST]
    index = [i for _, i in entries] + (rest if rest_last else [])
    out_values = [v for v, _ in entries] + ([0] * len(rest) if rest_last else [])
    return index, out_values, [cls[i] for i in index], sum(1 for c in cls if c == CARRIED), len(rest)


def values_of(data, offsets, ids, caps, parts, terms, K, formats=None):
    """(values per line -- an int or None --, numbers, unset, not_numbers).  formats: {(extraction, group): (kind, scale)} of
    number_oracle, absent: Long.parseLong."""
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
    values, unset, nan = [None] * len(oc), 0, 0
    for i in np.flatnonzero(keep):
        k = int(oc[i])
        g = group_of[k]
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        if not pair_set(b, e, off[i + 1] - off[i]):
            unset += 1
            continue
        units = data[off[i] + b:off[i] + e].tolist()
        v = NO.parse(*formats[k, g], units) if formats and (k, g) in formats else parse_long(units)
        if v is None:
            nan += 1
        else:
            values[i] = v
    numbers = sum(1 for v in values if v is not None)
    return values, numbers, unset, nan


def sort_lines(data, offsets, ids, caps, parts, terms, K, descending=False, carry=False, rest="drop", formats=None, all_digits=False):
    """What Gorp.sort_lines returns: index, values, line_class, data, offsets, ids, caps (None for compact rows: ids holds whole rows)
    and totals."""
    values, numbers, unset, nan = values_of(data, offsets, ids, caps, parts, terms, K, formats)
    index, out_values, out_class, carried, n_rest = order_of(values, carry, descending, rest == "last")
    off = np.asarray(offsets).astype(np.int64)
    lengths = off[1:] - off[:-1]
    idx = np.asarray(index, np.int64)
    pieces = [np.asarray(data)[off[i]:off[i + 1]] for i in index]
    m = numbers + carried
    stamped = [v for v in values if v is not None]
    keys = [key_of(v, descending) for v, c in zip(out_values, out_class) if c != REST]
    return {"index": index, "values": out_values, "line_class": out_class,
            "data": np.concatenate(pieces) if pieces else np.zeros(0, np.asarray(data).dtype),
            "offsets": np.concatenate([[0], np.cumsum(lengths[idx])]).astype(np.int64).tolist(),
            "ids": np.asarray(ids)[idx], "caps": None if caps is None or np.asarray(ids).ndim == 2 else np.asarray(caps)[idx],
            "totals": {"lines": numbers + unset + nan, "numbers": numbers, "unset": unset, "not_numbers": nan, "carried": carried, "rest": n_rest,
                       "lines_out": len(index), "units_out": int(lengths[idx].sum()), "first_value": out_values[0] if m else 0,
                       "last_value": out_values[m - 1] if m else 0, "n_passes": len(plan(keys, all_digits)),
                       "already_ordered": all((b >= a) != descending or a == b for a, b in zip(stamped, stamped[1:]))}}


def same(got, want, data_dtype=np.uint8, offsets_dtype=np.uint32):
    """Gorp.sort_lines' dict against sort_lines': every field, bit for bit."""
    assert got["totals"] == want["totals"], (got["totals"], want["totals"])
    assert got["index"].dtype == np.uint32 and got["index"].tolist() == want["index"]
    assert got["values"].dtype == np.int64 and got["values"].tolist() == want["values"]
    assert got["line_class"].dtype == np.uint8 and got["line_class"].tolist() == want["line_class"]
    assert got["data"].dtype == data_dtype and np.array_equal(got["data"], want["data"])
    assert got["offsets"].dtype == offsets_dtype and got["offsets"].tolist() == want["offsets"]
    if "ids" in got:
        assert got["ids"].dtype == want["ids"].dtype and np.array_equal(got["ids"], want["ids"])
        assert (got["caps"] is None) == (want["caps"] is None)
        if want["caps"] is not None:
            assert got["caps"].dtype == np.int32 and np.array_equal(got["caps"], want["caps"])
    return True


# ---------------------------------------------------------------------------
# the large case: values per line as int64 and a `stamped` mask
# ---------------------------------------------------------------------------
def np_sort(values, stamped, carry=False, descending=False, rest_last=False):
    """(index uint32, out_values int64, out_class uint8) with numpy alone: the nearest earlier stamped line by a running maximum of
    the stamped lines' numbers (the forward fill), one stable argsort of the entries' keys, the rest lines behind."""
    values, stamped = np.asarray(values, np.int64), np.asarray(stamped, bool)
    n = len(values)
    header = np.maximum.accumulate(np.where(stamped, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    cls = np.where(stamped, STAMPED, np.where((header >= 0) & carry, CARRIED, REST)).astype(np.uint8)
    entry = np.flatnonzero(cls != REST)
    filled = values[header[entry]]
    keys = filled.view(np.uint64) ^ np.uint64(2 ** 63)
    if descending:
        keys = ~keys
    by = np.argsort(keys, kind="stable")
    rest = np.flatnonzero(cls == REST) if rest_last else np.zeros(0, np.int64)
    index = np.concatenate([entry[by], rest])
    return index.astype(np.uint32), np.concatenate([filled[by], np.zeros(len(rest), np.int64)]), cls[index]
