"""The rule of gx_group_quantiles restated in Python, for the tests of both sides (tests/test_group_quantile_host.py: the digit plan,
the host sort and the pick of gx_group_quantile.hpp as a program under sanitizers; tests/test_gpu_group_quantile.py: the kernels).
The keys, line_key and the stats are group_oracle.group_lines'; key j's population is the numbers among key j's lines whose part has a
value group (where_oracle.pair_set, where_oracle.parse_long); per key the rows are quantile_oracle.quantiles_of over that population."""
import numpy as np

from group_oracle import NONE, group_lines, same
from quantile_oracle import quantiles_of
from where_oracle import outcome, pair_set, parse_long, unpack

DIGIT_BITS, VALUE_DIGITS = 6, 11


def populations(data, offsets, ids, caps, parts, K, line_key, n_keys):
    """per key, the numbers of its lines in line order"""
    data = np.asarray(data)
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    value_group = {k: v for k, _, v in parts}
    pops = [[] for _ in range(n_keys)]
    for i, j in enumerate(line_key):
        if j == NONE:
            continue
        g = value_group[int(oc[i])]
        if g < 0:
            continue
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        if not pair_set(b, e, off[i + 1] - off[i]):
            continue
        v = parse_long(data[off[i] + b:off[i] + e].tolist())
        if v is not None:
            pops[j].append(v)
    return pops


def group_quantiles(data, offsets, ids, caps, parts, terms, K, asks):
    """What gx_group_quantiles delivers: group_oracle.group_lines' dict plus "quantiles", per key a list of quantiles_of's dicts, and
    "populations" for the tests' own cross-checks."""
    want = group_lines(data, offsets, ids, caps, parts, terms, K)
    pops = populations(data, offsets, ids, caps, parts, K, want["line_key"], len(want["keys"]))
    if want["stats"] is not None:
        assert [len(p) for p in pops] == [s["numbers"] for s in want["stats"]]
    want["populations"] = pops
    want["quantiles"] = [quantiles_of(p, asks) for p in pops]
    return want


def same_quantiles(got, want, asks, data_dtype=np.uint8):
    """Gorp.group_quantiles' dict against group_quantiles': group_oracle.same, then every row bit for bit and the invariants."""
    same(got, want, data_dtype)
    assert got["quantiles"] == want["quantiles"], [(j, g, w) for j, (g, w) in enumerate(zip(got["quantiles"], want["quantiles"])) if g != w][:3]
    check_invariants(got, asks)
    return True


def check_invariants(got, asks=None):
    """below < rank <= below + equal <= numbers; num == 0 is the minimum and num == den the maximum of key_stats"""
    for j, rows in enumerate(got["quantiles"]):
        numbers = got["stats"][j]["numbers"] if got["stats"] is not None else 0
        for q, r in enumerate(rows):
            if numbers == 0:
                assert r == {"value": None, "rank": 0, "below": 0, "equal": 0}, (j, q, r)
                continue
            assert r["below"] < r["rank"] <= r["below"] + r["equal"] <= numbers, (j, q, r, numbers)
            if asks is not None and asks[q][0] == 0:
                assert r["value"] == got["stats"][j]["min"] and r["rank"] == 1 and r["below"] == 0
            if asks is not None and asks[q][0] == asks[q][1]:
                assert r["value"] == got["stats"][j]["max"] and r["rank"] == numbers and r["below"] + r["equal"] == numbers


# ---------------------------------------------------------------------------
# the digit plan (gx_group_quantile.hpp: gq_key_bits, gq_plan), for the program under sanitizers
# ---------------------------------------------------------------------------
def key_of(v):
    return v + 2 ** 63


def key_bits(n_keys):
    return (n_keys - 1).bit_length() if n_keys > 1 else 0


def plan_of(values, n_keys, all_values=False):
    """(the value digits sorted as a bit mask, the key digits sorted, the buffer that holds the result): a value digit is sorted
    exactly when two candidates differ in it"""
    mask = 0
    for d in range(VALUE_DIGITS):
        if all_values or len({(key_of(v) >> (DIGIT_BITS * d)) & 63 for v in values}) > 1:
            mask |= 1 << d
    key_digits = -(-key_bits(n_keys) // DIGIT_BITS)
    return mask, key_digits, (bin(mask).count("1") + key_digits) & 1
