"""The rule of gx_capture_quantiles restated in Python, for the tests of both sides (tests/test_quantile_host.py: the C++ rule as a
program under sanitizers; tests/test_gpu_quantile.py: the kernels).  Every line is classed as tests/top_oracle.py classes one -- it
counts when its outcome is an extraction that has a part and every term of that extraction holds; its value is unset, no number or a
number -- and a quantile num / den of the numbers is sorted(values)[rank - 1] with the nearest rank ceil(num * numbers / den), at
least 1, plus the counts of the numbers below and equal to that value."""
import math
from fractions import Fraction

import numpy as np

from where_oracle import keep_lines, outcome, pair_set, parse_long, unpack


def rank_of(num, den, numbers):
    """1 <= rank <= numbers (0 without numbers), by exact rational arithmetic"""
    return max(1, math.ceil(Fraction(num, den) * numbers)) if numbers else 0


def quantiles_of(values, asks):
    """values: the population, in any order (a list of ints or an int64 array); asks: [(num, den)].  One dict per ask, in order."""
    v = np.sort(np.asarray(values, dtype=np.int64)) if len(values) else np.zeros(0, np.int64)
    out = []
    for num, den in asks:
        if not len(v):
            out.append({"value": None, "rank": 0, "below": 0, "equal": 0})
            continue
        r = rank_of(num, den, len(v))
        x = v[r - 1]
        below = int(np.searchsorted(v, x, side="left"))
        out.append({"value": int(x), "rank": r, "below": below, "equal": int(np.searchsorted(v, x, side="right")) - below})
    return out


def population(data, offsets, ids, caps, parts, terms, K):
    """(values in line order, unset, not_numbers).  ids: int32 match ids and caps their dense rows, or ids = u16 / u8 result rows (caps
    None); parts: top_oracle.decode_parts'; terms: where_oracle.decode_terms'."""
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
    values, unset, nan = [], 0, 0
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
            values.append(v)
    return values, unset, nan


def capture_quantiles(data, offsets, ids, caps, parts, terms, K, asks):
    """What Gorp.capture_quantiles returns: (results, totals)."""
    values, unset, nan = population(data, offsets, ids, caps, parts, terms, K)
    return quantiles_of(values, asks), {"lines": len(values) + unset + nan, "numbers": len(values), "unset": unset, "not_numbers": nan}


# ---------------------------------------------------------------------------
# populations and quantiles that both sides' tests run
# ---------------------------------------------------------------------------
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
D32 = 2 ** 32 - 1
# 16 quantiles: the ends, repeats, den = 1, den = 2^32 - 1
ASKS = [(0, 1), (1, 1), (1, 2), (1, 2), (95, 100), (99, 100), (1, 3), (D32 - 1, D32), (1, D32), (0, D32), (7, 7), (0, 5), (1, 4), (3, 4), (1, 255), (254, 255)]
SIXTEENTHS = [(j + 1, 16) for j in range(16)]


def key_of(v):
    """gx_top.hpp: top_key(v, false)"""
    return v + 2 ** 63


def groups_before_digits(values_found):
    """The number of groups before each of the eight digits, most significant first, for quantiles that find these values."""
    return [len({key_of(v) >> (8 * (d + 1)) for v in values_found}) for d in range(7, -1, -1)]


def parting_values():
    """16 values, ascending, whose keys part at every one of the eight digits: the highest differs from the rest in digit 7 alone (and
    is the only one that is not negative), the next in digit 6, ... the tenth in digit 1, and the lowest nine in digit 0."""
    keys = []
    for j in range(16):
        k = 0x7F << 56
        if j == 15:
            k = 0x80 << 56
        elif j >= 9:
            k |= 1 << (8 * (j - 8))
        else:
            k |= j
        keys.append(k)
    values = [k - 2 ** 63 for k in keys]
    assert values == sorted(values) and groups_before_digits(values) == [1, 2, 3, 4, 5, 6, 7, 8]
    return values


def rule_cases():
    """[(values, asks)]: the edges of int64, equal values, one digit at a time, small populations, parting prefixes"""
    base = 0x0102030405060708
    cases = [([INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MIN + 1, INT64_MAX - 1, -256, 255, -2 ** 32, 2 ** 32, INT64_MIN, INT64_MAX], ASKS),
             ([-5, -3, -3, -1000000, -7, -7, -7, -1], ASKS),
             ([42] * 100, ASKS),
             ([7, -7] * 50 + [7], ASKS),
             ([7], ASKS), ([INT64_MIN], ASKS), ([3, -3], ASKS),
             ([(i * 37) % 255 - 100 for i in range(255)], ASKS)]
    for d in (7, 0):   # values that differ in one byte of the key alone
        digits = [(i * 101) % 256 for i in range(256)] + [(i * 7) % 256 for i in range(100)]
        cases.append(([((base & ~(0xFF << (8 * d))) | (x << (8 * d))) - 2 ** 63 for x in digits], ASKS))
    parting = parting_values()
    cases.append((parting[::-1], SIXTEENTHS))
    cases.append(([v for v in parting for _ in range(3)][::-1], SIXTEENTHS))
    cases.append((parting, [(1, 2)] * 16))                       # all quantiles equal
    cases.append(([5, 1, 4], []))                                # no quantiles
    cases.append(([], ASKS))                                     # no numbers
    return cases
