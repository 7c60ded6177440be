"""The rule of gx_group_pairs restated in Python, for the tests of both sides (tests/test_pairs_host.py: the pair hash and the
find-or-insert of gx_pairs.hpp as a program under sanitizers; tests/test_gpu_pairs.py: the kernels): group_oracle.group_lines for the
keys, then a dict keyed by (line_key[i], second tuple) filled line by line, whose insertion order is the order of the pairs.  A keyed
line is paired when its part has a second group and that group's capture names a value (where_oracle.pair_set).  np_pairs is the numpy
restatement for the large case -- first-appearance numbering by a minimum-scatter, no np.unique -- which test_pairs_host.py compares
with the oracle on small draws of the same generator."""
import numpy as np

from group_oracle import M64, NONE, group_lines, hash_units
from group_oracle import same as same_group
from where_oracle import outcome, pair_set, unpack

PAIR_TOTALS = ("n_pairs", "pair_units", "paired", "unpaired", "pairs_exact")


def decode_seconds(seconds, n):
    """Gorp.pair_parts' second groups as a list of ints (-1: none)."""
    return [int(seconds[t]) for t in range(n)]


def group_pairs(data, offsets, ids, caps, parts, seconds, terms, K):
    """What gx_group_pairs delivers.  ids / caps / parts / terms as group_oracle.group_lines takes them; seconds: per part its second group
    or -1.  Returns group_lines' dict plus pairs (a list of (key number, second tuple)), pair_first_line, pair_lines, key_pairs,
    line_pair, and the pair totals in totals."""
    want = group_lines(data, offsets, ids, caps, parts, terms, K)
    if np.asarray(ids).ndim == 2:
        ids, caps = unpack(ids)
    oc = outcome(ids, K)
    off = np.asarray(offsets).astype(np.int64)
    second_of = {k: s for (k, _, _), s in zip(parts, seconds)}
    number, pairs, first, count, line_pair = {}, [], [], [], []
    unpaired = 0
    for i, j in enumerate(want["line_key"]):
        if j == NONE:
            line_pair.append(NONE)
            continue
        s = second_of[int(oc[i])]
        value = None
        if s >= 0:
            b, e = int(caps[i, 2 * s]), int(caps[i, 2 * s + 1])
            if pair_set(b, e, off[i + 1] - off[i]):
                value = tuple(np.asarray(data)[off[i] + b:off[i] + e].tolist())
        if value is None:
            unpaired += 1
            line_pair.append(NONE)
            continue
        if (j, value) not in number:
            number[j, value] = len(pairs)
            pairs.append((j, value))
            first.append(i)
            count.append(0)
        count[number[j, value]] += 1
        line_pair.append(number[j, value])
    key_pairs = [0] * len(want["keys"])
    for j, _ in pairs:
        key_pairs[j] += 1
    want.update(pairs=pairs, pair_first_line=first, pair_lines=count, key_pairs=key_pairs, line_pair=line_pair)
    want["totals"] = dict(want["totals"], n_pairs=len(pairs), pair_units=sum(len(v) for _, v in pairs), paired=sum(count), unpaired=unpaired, pairs_exact=True)
    assert want["totals"]["keyed"] == want["totals"]["paired"] + unpaired
    return want


def same(got, want, data_dtype=np.uint8, offsets_dtype=np.uint32):
    """Gorp.group_pairs' dict (keys="csr") against group_pairs': every field and dtype, bit for bit."""
    assert {k: got["totals"][k] for k in PAIR_TOTALS} == {k: want["totals"][k] for k in PAIR_TOTALS}, (got["totals"], want["totals"])
    group = lambda d: dict(d, totals={k: v for k, v in d["totals"].items() if k not in PAIR_TOTALS})
    same_group(group(got), group(want), data_dtype)
    p = len(want["pairs"])
    poff, units = np.asarray(got["pair_offsets"]), np.asarray(got["pair_units"])
    assert units.dtype == data_dtype and poff.dtype == offsets_dtype and len(poff) == p + 1 and poff[0] == 0 and poff[-1] == len(units) == want["totals"]["pair_units"]
    assert got["pair_key"].dtype == np.uint32 and len(got["pair_key"]) == p
    assert [(int(got["pair_key"][j]), tuple(units[int(poff[j]):int(poff[j + 1])].tolist())) for j in range(p)] == want["pairs"]
    assert got["pair_first_line"].dtype == np.uint32 and got["pair_first_line"].tolist() == want["pair_first_line"]
    assert got["pair_lines"].dtype == np.uint64 and got["pair_lines"].tolist() == want["pair_lines"]
    assert got["key_pairs"].dtype == np.uint64 and got["key_pairs"].tolist() == want["key_pairs"]
    assert got["line_pair"].dtype == np.uint32 and got["line_pair"].tolist() == want["line_pair"]
    assert sorted(want["pair_first_line"]) == want["pair_first_line"] and sum(want["key_pairs"]) == p
    return True


# ---------------------------------------------------------------------------
# batches for a handle of K identical extractions `a(.*)(.*)...`: group 0 the key, group 1 the second
# ---------------------------------------------------------------------------
def batch(keys, seconds, lengths=None, ids=None, dtype=np.uint8, offsets_dtype=np.uint32, groups=2, filler=0x2E):
    """A line is its key, its second (sequences of code units; None: that group is unset) and filler up to lengths[i] units.  Returns
    (data, offsets, ids, caps): group 0 is the key, group 1 the second, further groups unset."""
    n = len(keys)
    klen = np.array([0 if k is None else len(k) for k in keys], np.int64)
    slen = np.array([0 if s is None else len(s) for s in seconds], np.int64)
    lens = klen + slen if lengths is None else np.maximum(np.asarray(lengths, np.int64), klen + slen)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(offsets_dtype)
    data = np.full(int(lens.sum()), filler, dtype)
    caps = np.full((n, 2 * groups), -1, np.int32)
    for i in range(n):
        o = int(offsets[i])
        if keys[i] is not None:
            data[o:o + klen[i]] = np.frombuffer(keys[i], np.uint8) if isinstance(keys[i], bytes) else keys[i]
            caps[i, 0], caps[i, 1] = 0, klen[i]
        if seconds[i] is not None:
            data[o + klen[i]:o + klen[i] + slen[i]] = np.frombuffer(seconds[i], np.uint8) if isinstance(seconds[i], bytes) else seconds[i]
            caps[i, 2], caps[i, 3] = klen[i], klen[i] + slen[i]
    return data, offsets, np.zeros(n, np.int32) if ids is None else np.asarray(ids, np.int32), caps


def draw(n_lines, n_keys, n_seconds, seed, no_key=0.05, no_second=0.05):
    """(key names, second names, extra): per line a key name in [0, n_keys) or -1 (no key: a share of no_key), a second name in
    [0, n_seconds) or -1 (unset: a share of no_second) and 0 .. 5 units of filler"""
    rng = np.random.default_rng(seed)
    kn = rng.integers(0, n_keys, n_lines)
    sn = rng.integers(0, n_seconds, n_lines)
    kn[rng.random(n_lines) < no_key] = -1
    sn[rng.random(n_lines) < no_second] = -1
    return kn.astype(np.int64), sn.astype(np.int64), rng.integers(0, 6, n_lines).astype(np.int64)


def named_batch(kn, sn, extra):
    """draw()'s names as a batch built by numpy alone: a line is the key name's two bytes (big-endian), the second name's one byte and
    `extra` bytes of filler; no key: unmatched; no second: group 1 unset (its byte is filler, or not there at all with extra = -1)."""
    n = len(kn)
    lens = 3 + np.asarray(extra, np.int64)
    assert ((lens >= 3) | ((lens == 2) & (sn < 0))).all()
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = np.full(int(offsets[-1]), 0x2E, np.uint8)
    at = offsets[:-1].astype(np.int64)
    data[at] = (np.maximum(kn, 0) >> 8) & 255
    data[at + 1] = np.maximum(kn, 0) & 255
    data[at[sn >= 0] + 2] = sn[sn >= 0] & 255
    ids = np.where(kn < 0, -1, 0).astype(np.int32)
    caps = np.tile(np.array([0, 2, 2, 3], np.int32), (n, 1))
    caps[sn < 0, 2:] = -1
    return data, offsets, ids, caps


def number_by_first(names):
    """names[n] (int64, -1: none) numbered by first appearance with numpy alone: (number per line or NONE, first line per number, lines
    per number)"""
    names = np.asarray(names, np.int64)
    has = names >= 0
    if not has.any():
        return np.full(len(names), NONE, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    top = int(names.max()) + 1
    first = np.full(top, len(names), np.int64)
    np.minimum.at(first, names[has], np.flatnonzero(has))
    seen = np.flatnonzero(first < len(names))
    by_first = seen[np.argsort(first[seen], kind="stable")]
    number = np.full(top, -1, np.int64)
    number[by_first] = np.arange(len(by_first))
    line = np.where(has, number[np.where(has, names, 0)], NONE)
    return line, first[by_first], np.bincount(line[has], minlength=len(by_first))


def np_pairs(kn, sn, n_seconds):
    """draw()'s names -> (line_key, key_lines, line_pair, pair_key, pair_first_line, pair_lines, key_pairs) with numpy alone"""
    kn, sn = np.asarray(kn, np.int64), np.asarray(sn, np.int64)
    line_key, _, key_lines = number_by_first(kn)
    both = np.where((kn >= 0) & (sn >= 0), kn * n_seconds + sn, -1)
    line_pair, pair_first, pair_lines = number_by_first(both)
    pair_key = line_key[pair_first]
    key_pairs = np.bincount(pair_key, minlength=len(key_lines)) if len(pair_key) else np.zeros(len(key_lines), np.int64)
    return (line_key.astype(np.uint32), key_lines.astype(np.uint64), line_pair.astype(np.uint32), pair_key.astype(np.uint32), pair_first.astype(np.uint32),
            pair_lines.astype(np.uint64), key_pairs.astype(np.uint64))


# ---------------------------------------------------------------------------
# the pair table itself (gx_pairs.hpp), for the program under sanitizers
# ---------------------------------------------------------------------------
def pair_hash(units, key_slot, weak=False):
    """gx_pairs.hpp's pair_hash of group_hash(units) and the key slot"""
    h = hash_units(units) ^ (((key_slot + 1) * 0x9E3779B97F4A7C15) & M64)
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h & 7 if weak else h


def probe_pairs(items, slots, weak=False):
    """items: (key slot, second units).  Linear probing from hash & (slots - 1): per item (its slot or None ("full"), the slots it
    loaded), and the table as {slot: (line, tag)}."""
    table, held, out = {}, {}, []
    for i, (k, v) in enumerate(items):
        h = pair_hash(v, k, weak)
        s, found, loads = h & (slots - 1), None, 0
        for _ in range(slots):
            loads += 1
            if s not in table:
                table[s], held[s] = (i, h >> 32), (k, tuple(v))
                found = s
                break
            if held[s] == (k, tuple(v)):
                found = s
                break
            s = (s + 1) & (slots - 1)
        out.append((found, loads))
    return out, table
