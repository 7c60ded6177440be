"""The rule of gx_top_groups restated in Python, for the tests of both sides (tests/test_top_groups_host.py: the key map, digit plan
and select of gx_top_groups.hpp as a program under sanitizers; tests/test_gpu_top_groups.py: the kernels): group_oracle.group_lines,
a rank value per key as a Python int, and sorted() by (-value, key number)."""
import numpy as np

from group_oracle import NONE, group_lines

RANK_BY = ("lines", "numbers", "sum", "max", "min")
TOP_GROUPS_MAX = 4096
M64 = 2 ** 64 - 1
M128 = 2 ** 128 - 1


def rank_values(grouped, by):
    """[(key number, rank value)] of the candidates, in key-number order."""
    n_keys = len(grouped["keys"])
    if by == "lines":
        return [(j, grouped["lines"][j]) for j in range(n_keys)]
    stats = grouped["stats"]
    assert stats is not None, "ranking by numbers needs a part with a value group"
    if by == "numbers":
        return [(j, stats[j]["numbers"]) for j in range(n_keys)]
    return [(j, stats[j][by]) for j in range(n_keys) if stats[j]["numbers"] >= 1]


def rank(candidates, n_wanted, largest=True):
    """candidates: [(key number, value)] -> (the chosen ones in rank order, last value or None, ties_left)"""
    ordered = sorted(candidates, key=lambda c: ((-c[1] if largest else c[1]), c[0]))
    top = ordered[:n_wanted]
    if not top:
        return top, None, 0
    last = top[-1][1]
    return top, last, sum(1 for _, v in candidates if v == last) - sum(1 for _, v in top if v == last)


def top_groups(data, offsets, ids, caps, parts, terms, K, n_wanted, by="lines", largest=True):
    """What gx_top_groups delivers, as Gorp.top_groups' dict (keys: tuples of code units)."""
    g = group_lines(data, offsets, ids, caps, parts, terms, K)
    cand = rank_values(g, by)
    top, last, ties_left = rank(cand, n_wanted, largest)
    order = [j for j, _ in top]
    rank_of = {j: r for r, j in enumerate(order)}
    return {"keys": [g["keys"][j] for j in order], "key_number": order, "first_line": [g["first_line"][j] for j in order],
            "lines": [g["lines"][j] for j in order], "stats": None if g["stats"] is None else [g["stats"][j] for j in order],
            "line_rank": [NONE if j == NONE else rank_of.get(j, NONE) for j in g["line_key"]], "values": [v for _, v in top],
            "totals": {"group": g["totals"], "candidates": len(cand), "n_top": len(top), "units_top": sum(len(g["keys"][j]) for j in order),
                       "last": last, "ties_left": ties_left},
            "grouped": g, "candidates": cand}


def same(got, want, n_wanted, largest=True, data_dtype=np.uint8):
    """Gorp.top_groups' dict (keys="csr") against top_groups': every field bit for bit, and the invariants."""
    t, k = want["totals"], want["totals"]["n_top"]
    assert got["totals"] == t, (got["totals"], t)
    assert t["n_top"] == min(n_wanted, t["candidates"]) and t["group"] == want["grouped"]["totals"]
    koff = np.asarray(got["key_offsets"]).astype(np.int64)
    units = np.asarray(got["key_units"])
    assert units.dtype == data_dtype and len(koff) == k + 1 and koff[0] == 0 and koff[-1] == len(units) == t["units_top"]
    assert [tuple(units[koff[r]:koff[r + 1]].tolist()) for r in range(k)] == want["keys"]
    for name, dtype in (("key_number", np.uint32), ("first_line", np.uint32), ("lines", np.uint64)):
        assert np.asarray(got[name]).dtype == dtype and np.asarray(got[name]).tolist() == want[name], name
    if "line_rank" in got:
        assert np.asarray(got["line_rank"]).dtype == np.uint32 and np.asarray(got["line_rank"]).tolist() == want["line_rank"]
    assert (got["stats"] is None) == (want["stats"] is None)
    if want["stats"] is not None:
        assert len(got["stats"]) == k
        for r, (g, w) in enumerate(zip(got["stats"], want["stats"])):
            assert g["lines"] == g["numbers"] + g["unset"] + g["not_numbers"], (r, g)
            assert g == w, (r, g, w)
    # the order is strict: (value, key number) never repeats and never goes back
    sign = -1 if largest else 1
    pairs = [(sign * v, j) for v, j in zip(want["values"], want["key_number"])]
    assert all(a < b for a, b in zip(pairs, pairs[1:]))
    # below + ties: the candidates strictly better than `last` are all delivered; of those equal to it, the delivered ones and ties_left
    if k:
        last = t["last"]
        better = sum(1 for _, v in want["candidates"] if sign * v < sign * last)
        equal = sum(1 for _, v in want["candidates"] if v == last)
        assert better + equal - t["ties_left"] == k and 0 <= t["ties_left"] < equal
    else:
        assert t["last"] is None and t["ties_left"] == 0
    return True


# ---------------------------------------------------------------------------
# the header's pieces (gx_top_groups.hpp), for the program under sanitizers
# ---------------------------------------------------------------------------
def key_of(value, smallest=False):
    """the order-preserving unsigned 128-bit key of a signed 128-bit value: sign bit flipped, complemented for smallest"""
    k = (value & M128) ^ (1 << 127)
    return (~k & M128) if smallest else k


def plan_of(values, smallest=False):
    """bit d set: two of the values' keys differ in 8-bit digit d (0: the least significant)"""
    keys = [key_of(v, smallest) for v in values]
    if not keys:
        return 0
    o = a = keys[0]
    for k in keys[1:]:
        o |= k
        a &= k
    differ = o ^ a
    return sum(1 << d for d in range(16) if (differ >> (8 * d)) & 0xFF)


# ---------------------------------------------------------------------------
# large fabricated batches: a generator that leaves no case out, and a numpy restatement
# ---------------------------------------------------------------------------
def skewed_draw(n_lines, n_names, seed):
    """(key name per line, int64 value per line): names drawn skewed -- a few names hold most lines, the tail one or two each, so the
    counts repeat -- and values small enough that every sum fits an int64 (the numpy restatement sums in int64).  Every line has a key
    and a number, so every draw is one the restatements can state: none is left out."""
    rng = np.random.default_rng(seed)
    names = np.minimum((n_names * rng.random(n_lines) ** 3).astype(np.int64), n_names - 1)
    values = rng.integers(-10 ** 6, 10 ** 6, n_lines)
    return names, values


def np_top(names, values, n_wanted, by, largest=True):
    """The restatement for batches where every line has a key and a number: the keys numbered by first appearance, the rank value per key
    with numpy, np.lexsort on (key number, -value).  Returns (key numbers in rank order, their rank values, n_keys, ties_left)."""
    names, values = np.asarray(names), np.asarray(values, np.int64)
    uniq, first, inverse = np.unique(names, return_index=True, return_inverse=True)
    number = np.empty(len(uniq), np.int64)
    number[np.argsort(first)] = np.arange(len(uniq))
    knum = number[inverse]
    n_keys = len(uniq)
    if by in ("lines", "numbers"):
        v = np.bincount(knum, minlength=n_keys).astype(np.int64)
    elif by == "sum":
        v = np.zeros(n_keys, np.int64)
        np.add.at(v, knum, values)
    elif by == "max":
        v = np.full(n_keys, np.iinfo(np.int64).min)
        np.maximum.at(v, knum, values)
    else:
        v = np.full(n_keys, np.iinfo(np.int64).max)
        np.minimum.at(v, knum, values)
    order = np.lexsort((np.arange(n_keys), -v if largest else v))[:n_wanted]
    ties_left = int((v == v[order[-1]]).sum() - (v[order] == v[order[-1]]).sum()) if len(order) else 0
    return order, v[order], n_keys, ties_left
