"""The rule of gx_lines_by_key restated in Python, for the tests of both sides (tests/test_by_key_host.py: the keep rule, the digit plan and
the sort of gx_by_key.hpp as a program under sanitizers; tests/test_gpu_by_key.py: the kernels): group_oracle.group_lines for the keys,
the keep rule per key, sorted(kept lines, key=(line_key[i], i)), the two prefixes and the gathered batch.  np_by_key is the numpy
restatement for the large case -- first-appearance numbering plus a stable argsort, no np.unique -- which test_by_key_host.py compares
with the oracle on small draws of the same generator."""
import numpy as np

from group_oracle import NONE, group_lines
from group_oracle import same as same_group

BY_KEY_MAX_PASSES = 5


def kept(lines, min_lines=1, max_lines=None):
    """the keep rule: max(min_lines, 1) <= lines, and no max_lines (None or 0) or lines <= max_lines"""
    return lines >= max(min_lines, 1) and (not max_lines or lines <= max_lines)


def passes(n_keys, all_digits=False):
    """six-bit digits of the key numbers 0 .. n_keys - 1: ceil(bits(n_keys - 1) / 6), none for one key (and for none)"""
    return BY_KEY_MAX_PASSES if all_digits else (max(n_keys - 1, 0).bit_length() + 5) // 6


def regroup(line_key, key_lines, lengths, min_lines=1, max_lines=None):
    """(order, key_out_lines, key_out_units): the kept lines by (key number, line), and per key the exclusive prefixes."""
    keep = [kept(c, min_lines, max_lines) for c in key_lines]
    order = sorted((i for i, j in enumerate(line_key) if j != NONE and keep[j]), key=lambda i: (line_key[i], i))
    lines_of, units_of = [0] * len(key_lines), [0] * len(key_lines)
    for i in order:
        lines_of[line_key[i]] += 1
        units_of[line_key[i]] += int(lengths[i])
    kol, kou = [0], [0]
    for j in range(len(key_lines)):
        assert lines_of[j] == (key_lines[j] if keep[j] else 0)
        kol.append(kol[-1] + lines_of[j])
        kou.append(kou[-1] + units_of[j])
    return order, kol, kou


def lines_by_key(data, offsets, ids, caps, parts, terms, K, min_lines=1, max_lines=None):
    """What gx_lines_by_key delivers: group_oracle.group_lines' dict plus index, data, offsets, ids, caps (None for compact rows: ids
    holds whole rows), key_out_lines, key_out_units, and totals with keys_kept, lines_out, units_out."""
    want = group_lines(data, offsets, ids, caps, parts, terms, K)
    off = np.asarray(offsets).astype(np.int64)
    lengths = off[1:] - off[:-1]
    order, kol, kou = regroup(want["line_key"], want["lines"], lengths, min_lines, max_lines)
    idx = np.asarray(order, np.int64)
    pieces = [np.asarray(data)[off[i]:off[i + 1]] for i in order]
    want["index"] = order
    want["data"] = np.concatenate(pieces) if pieces else np.zeros(0, np.asarray(data).dtype)
    want["offsets"] = np.concatenate([[0], np.cumsum(lengths[idx])]).astype(np.int64).tolist()
    want["ids"] = np.asarray(ids)[idx]
    want["caps"] = None if caps is None or np.asarray(ids).ndim == 2 else np.asarray(caps)[idx]
    want["key_out_lines"], want["key_out_units"] = kol, kou
    want["totals"] = dict(want["totals"], keys_kept=sum(1 for c in want["lines"] if kept(c, min_lines, max_lines)), lines_out=len(order), units_out=kou[-1])
    return want


def same(got, want, data_dtype=np.uint8, offsets_dtype=np.uint32):
    """Gorp.lines_by_key's dict against lines_by_key's: every field, bit for bit."""
    assert {k: got["totals"][k] for k in ("keys_kept", "lines_out", "units_out")} == {k: want["totals"][k] for k in ("keys_kept", "lines_out", "units_out")}, got["totals"]
    group = lambda d: dict(d, totals={k: v for k, v in d["totals"].items() if k not in ("keys_kept", "lines_out", "units_out")})
    same_group(group(got), group(want), data_dtype)
    assert got["index"].dtype == np.uint32 and got["index"].tolist() == want["index"]
    assert got["data"].dtype == data_dtype and np.array_equal(got["data"], want["data"])
    assert got["offsets"].dtype == offsets_dtype and got["offsets"].tolist() == want["offsets"]
    if "ids" in got:
        assert got["ids"].dtype == want["ids"].dtype and np.array_equal(got["ids"], want["ids"])
        assert (got["caps"] is None) == (want["caps"] is None)
        if want["caps"] is not None:
            assert got["caps"].dtype == np.int32 and np.array_equal(got["caps"], want["caps"])
    for name in ("key_out_lines", "key_out_units"):
        assert got[name].dtype == np.uint64 and got[name].tolist() == want[name], name
    k = want["totals"]["n_keys"]
    assert len(want["key_out_lines"]) == k + 1 and want["key_out_lines"][k] == want["totals"]["lines_out"] and want["key_out_units"][k] == want["totals"]["units_out"]
    return True


# ---------------------------------------------------------------------------
# the large case: names per line (-1: no key), lengths per line
# ---------------------------------------------------------------------------
def draw(n_lines, n_names, seed, no_key=0.05):
    """names[n_lines] (with n_lines >= n_names every name 0 .. n_names - 1 has a line that KEEPS it: exactly n_names keys; -1: a line
    without a key, a share of no_key of the other lines) and lengths"""
    rng = np.random.default_rng(seed)
    names = rng.integers(0, n_names, n_lines)
    placed = np.zeros(n_lines, bool)
    if n_lines >= n_names:
        at = rng.permutation(n_lines)[:n_names]
        names[at] = rng.permutation(n_names)
        placed[at] = True
    names[(rng.random(n_lines) < no_key) & ~placed] = -1
    assert n_lines < n_names or len(set(names[names >= 0].tolist())) == n_names
    return names.astype(np.int64), rng.integers(0, 6, n_lines).astype(np.int64)


def np_by_key(names, lengths, min_lines=1, max_lines=None):
    """(line_key uint32, key_lines, order, key_out_lines, key_out_units) with numpy alone: number the names by first appearance -- the
    first line of every name by a minimum-scatter, the names ordered by it -- then one stable argsort of the kept lines' key numbers."""
    names = np.asarray(names, np.int64)
    has = names >= 0
    top = int(names.max()) + 1 if has.any() else 0
    first = np.full(top, len(names), np.int64)
    np.minimum.at(first, names[has], np.flatnonzero(has))
    seen = np.flatnonzero(first < len(names))
    by_first = seen[np.argsort(first[seen], kind="stable")]
    number = np.full(top, -1, np.int64)
    number[by_first] = np.arange(len(by_first))
    line_key = np.where(has, number[np.where(has, names, 0)], NONE) if top else np.full(len(names), NONE, np.int64)
    key_lines = np.bincount(line_key[has], minlength=len(by_first)) if top else np.zeros(0, np.int64)
    keep_key = (key_lines >= max(min_lines, 1)) & ((key_lines <= max_lines) if max_lines else True)
    keep = has & keep_key[np.where(has, line_key, 0)] if top else has
    lines = np.flatnonzero(keep)
    order = lines[np.argsort(line_key[lines], kind="stable")]
    per_key = np.where(keep_key, key_lines, 0)
    units = np.bincount(line_key[order], weights=None if not len(order) else np.asarray(lengths)[order], minlength=len(by_first)).astype(np.int64)
    kol = np.concatenate([[0], np.cumsum(per_key)]).astype(np.uint64)
    kou = np.concatenate([[0], np.cumsum(units)]).astype(np.uint64)
    return line_key.astype(np.uint32), key_lines.astype(np.uint64), order.astype(np.uint32), kol, kou
