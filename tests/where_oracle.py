"""The rule of gx_select_lines_where restated in Python, for the tests of both sides (tests/test_where_host.py: the C++ rule as a
program under sanitizers; tests/test_gpu_where.py: the kernel): slice the value with the capture offsets, then ==, slices and
re.fullmatch(rb"[+-]?[0-9]+") plus a range check.  Values and literals are sequences of code units (ints); None is an unset group."""
import ctypes as C
import re

import numpy as np

from gorp_amd import _native as N

TEXT_OPS = [N.GX_WHERE_EQ, N.GX_WHERE_PREFIX, N.GX_WHERE_SUFFIX, N.GX_WHERE_CONTAINS]
INT_OPS = [N.GX_WHERE_INT_EQ, N.GX_WHERE_INT_LT, N.GX_WHERE_INT_LE, N.GX_WHERE_INT_GT, N.GX_WHERE_INT_GE]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
LITERAL_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 64, 255]
INT_TABLE = [b"0", b"-0", b"+5", b"007", b"00000000000000000000123", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
             b"-9223372036854775809", b"", b"-", b"+", b"--1", b"12a", b" 1", b"1 "]
INT_NUMBERS = [INT64_MIN, -1, 0, 1, INT64_MAX]


def parse_long(units):
    """Long.parseLong for ASCII input, or None."""
    if any(u > 0x7F for u in units) or not re.fullmatch(rb"[+-]?[0-9]+", bytes(units)):
        return None
    v = int(bytes(units))
    return v if INT64_MIN <= v <= INT64_MAX else None


def holds(op, negate, value, literal=(), number=0):
    value, literal = None if value is None else list(value), list(literal)
    if value is None:
        test = False
    elif op == N.GX_WHERE_SET:
        test = True
    elif op == N.GX_WHERE_EQ:
        test = value == literal
    elif op == N.GX_WHERE_PREFIX:
        test = value[:len(literal)] == literal
    elif op == N.GX_WHERE_SUFFIX:
        test = len(literal) <= len(value) and value[len(value) - len(literal):] == literal
    elif op == N.GX_WHERE_CONTAINS:
        test = any(value[at:at + len(literal)] == literal for at in range(len(value) - len(literal) + 1))
    else:
        v = parse_long(value)
        test = v is not None and {N.GX_WHERE_INT_EQ: v == number, N.GX_WHERE_INT_LT: v < number, N.GX_WHERE_INT_LE: v <= number,
                                  N.GX_WHERE_INT_GT: v > number, N.GX_WHERE_INT_GE: v >= number}[op]
    return test != bool(negate)


def pair_set(begin, end, line_units):
    return begin >= 0 and begin <= end <= line_units


def near_miss_cases(value_lengths, wide=False):
    """Literals of LITERAL_LENGTHS units against values: a hit at the start, in the middle, at the end; a miss in the last unit; a literal
    one unit longer than the value whose last unit lies just behind the capture's end."""
    rng = np.random.default_rng(7)
    top = 0x3000 if wide else 250
    cases = []
    for ln in LITERAL_LENGTHS:
        lit = tuple(int(x) for x in rng.integers(1, top, ln))
        miss = lit[:-1] + (lit[-1] ^ 1,) if ln else lit
        for vn in value_lengths:
            filler = [int(x) for x in rng.integers(top, top + 5, vn)]          # (no unit of the literal)
            for at in sorted({0, max(0, (vn - ln) // 2), max(0, vn - ln)}):
                if at + ln > vn:
                    continue
                for text in (lit, miss):
                    v = filler[:at] + list(text) + filler[at + ln:]
                    for op in TEXT_OPS:
                        cases.append((op, 0, tuple(v), 0, vn, lit, 0, wide))
            if ln and vn == ln - 1:
                # the value is the literal's first ln - 1 units, the literal's last unit is the line's next one
                for lead in (0, 3):
                    buf = tuple(filler[:lead]) + lit + (7,)
                    for op in TEXT_OPS:
                        cases.append((op, 0, buf, lead, lead + ln - 1, lit, 0, wide))
    return cases


# ---------------------------------------------------------------------------
# whole batches
# ---------------------------------------------------------------------------
def outcome(ids, K):
    v = np.asarray(ids, dtype=np.int64)
    oc = np.full(v.shape, 2 * K + 1, np.int64)
    oc = np.where((v >= 0) & (v < K), v, oc)
    oc = np.where(v == -1, K, oc)
    return np.where((v <= -2) & (v >= -1 - K), K + 1 + (-2 - v), oc)


def decode_terms(w):
    """Gorp.where_terms' result as [(extraction, group, op, negate, literal units, number)]."""
    out = []
    for t in list(w.array)[:w.n]:
        lit = []
        if t.text_units:
            ctype = C.c_uint16 if w.units == "utf-16" else C.c_uint8
            lit = np.ctypeslib.as_array(C.cast(t.text, C.POINTER(ctype)), (t.text_units,)).tolist()
        out.append((t.extraction, t.group, t.op, t.negate, lit, t.number))
    return out


def unpack(rows):
    """(ids, caps) of u16 / u8 result rows (gx_layout.hpp): the id signed, the all-ones unit -1."""
    rows = np.asarray(rows)
    unset = np.iinfo(rows.dtype).max
    ids = rows[:, 0].astype(np.int16 if rows.dtype == np.uint16 else np.int8).astype(np.int32)
    caps = np.where(rows[:, 1:] == unset, -1, rows[:, 1:].astype(np.int64)).astype(np.int32)
    return ids, caps


def keep_lines(data, offsets, ids, caps, mask, terms, K):
    """bool[n]: want[outcome] != 0 and, where the outcome is an extraction that has terms, every term holds.  ids: int32 match ids and caps
    their dense rows, or ids = u16 / u8 result rows (caps None); terms: decode_terms'."""
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    keep = np.append(np.asarray(mask, np.uint8), 0)[oc] != 0
    by_k = {}
    for t in terms:
        by_k.setdefault(t[0], []).append(t)
    off = np.asarray(offsets).astype(np.int64)
    for i in np.flatnonzero(keep & np.isin(oc, list(by_k))):
        for _, g, op, negate, lit, number in by_k[int(oc[i])]:
            b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
            value = data[off[i] + b:off[i] + e].tolist() if pair_set(b, e, off[i + 1] - off[i]) else None
            if not holds(op, negate, value, lit, number):
                keep[i] = False
                break
    return keep


def selection(data, offsets, keep):
    """(index, units, offsets) of the kept lines, as gx_select_lines writes them."""
    off = np.asarray(offsets).astype(np.int64)
    lens = off[1:] - off[:-1]
    index = np.flatnonzero(keep).astype(np.uint32)
    out_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.asarray(offsets).dtype)
    units = data[off[0]:off[-1]][np.repeat(keep, lens)]
    return index, units, out_off
