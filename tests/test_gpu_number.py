"""GPU tests of gx_set_number_format: every call that parses a captured value as a number parses it under its group's format.

Twin batches.  Batch A holds formatted values -- decimals, ISO 8601 and access-log stamps, drawn from number_oracle's case table and
from seeded random values.  Batch B holds the same lines with each value replaced here, on the host, by str(number) from
number_oracle.parse, or by `x` where it is no number; unset pairs stay unset.  The call on A, on a handle with the formats set, must
equal exactly the existing restatement (where_oracle, stats_oracle, group_oracle, top_oracle, quantile_oracle, group_quantile_oracle,
top_groups_oracle) applied to B, which knows no format.  Every field is compared; where an output carries line text it is compared
with A's own lines at the returned indices.  Batches are fabricated the way test_gpu_stats.py does it: ids and capture rows chosen
here, against a handle of K = 4 trivial extractions of 2 groups -- a line is its key followed by its value."""
import functools

import numpy as np
import pytest

import number_oracle as NO
from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import FlattenedExtraction, Gorp, parse_number
from group_oracle import decode_parts as group_parts_of
from group_oracle import group_lines
from group_oracle import same as same_groups
from group_quantile_oracle import group_quantiles, same_quantiles
from quantile_oracle import capture_quantiles
from stats_oracle import capture_stats, decode_measures, summarise
from stats_oracle import same as same_stats
from top_groups_oracle import same as same_top_groups
from top_groups_oracle import top_groups
from top_oracle import decode_parts as top_parts_of
from top_oracle import top_lines
from where_oracle import decode_terms, keep_lines, selection, unpack

pytestmark = pytest.mark.gpu

K = 4
KEY, VALUE = 0, 1                     # the groups of every extraction
FORMATS = {0: ("decimal", 3), 1: ("iso8601", 3), 2: ("iso8601", 9), 3: ("clf", 0)}   # of group VALUE; every KEY group is left LONG
ASKS = [(0, 1), (1, 2), (99, 100), (1, 1)]
SIZES = [1, 63, 64, 65, 1000]         # one lane; a wave less one, a wave, a wave and one; several waves in more than one workgroup


def construct():
    pieces = [["text", "a"], ["extractor", "key", [["pattern", ".*"]]], ["extractor", "value", [["pattern", ".*"]]]]
    g = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
    assert g.num_extractions == K and g.max_groups == 2
    return g


@functools.lru_cache(maxsize=None)
def handles():
    """(the handle with the formats set, one that was never given a format)"""
    formatted, plain = construct(), construct()
    for k, (kind, scale) in FORMATS.items():
        formatted.set_number_format(k, "value", kind, scale)
    return formatted, plain


@functools.lru_cache(maxsize=None)
def pools():
    """per extraction: values of its format -- the case table's texts of its kind, at whatever scale the table lists them, and random ones"""
    out = {}
    for k, (kind, scale) in FORMATS.items():
        code = NO.KINDS[kind]
        texts = sorted({text for kind2, _, text in NO.table() if kind2 == code and len(text) < 120})
        pool = texts + NO.random_values(code, scale, 3 * len(texts), 40 + k)
        # (a few of them in front: half of a batch's lines take one of these -- ties for the ranking calls, runs for the quantiles)
        common = [pool[int(j)] for j in np.random.default_rng(70 + k).choice(len(pool), 12, replace=False)]
        out[k] = common + pool
    return out


@functools.lru_cache(maxsize=None)
def twins(n, seed=1):
    """(lines A, lines B, ids, caps A, caps B, numbers): line = key + value; caps (0, key, key, end), or -1 pairs"""
    rng = np.random.default_rng(seed * 1000 + n)
    a_lines, b_lines, ids, a_caps, b_caps, numbers = [], [], [], [], [], []
    for i in range(n):
        k = int(rng.integers(-1, K)) if n > 1 else 1
        pool = pools()[max(k, 0)]
        value = pool[int(rng.integers(0, 12 if rng.integers(0, 2) else len(pool)))]
        key = b"%d" % int(rng.integers(0, 12))
        number = NO.parse(NO.KINDS[FORMATS[max(k, 0)][0]], FORMATS[max(k, 0)][1], value)
        twin = b"x" if number is None else b"%d" % number
        pick = int(rng.integers(0, 40)) if n > 1 else 9
        ka = kb = [0, len(key)]
        va, vb = [len(key), len(key) + len(value)], [len(key), len(key) + len(twin)]
        if pick == 0:
            va = vb = [-1, -1]                                  # the value group is unset
        elif pick == 1:
            ka = kb = [-1, -1]                                  # the key group is unset
        elif pick == 2:
            ka = kb = va = vb = [-1, -1]
        a_lines.append(key + value)
        b_lines.append(key + twin)
        ids.append(k)
        a_caps.append(ka + va)
        b_caps.append(kb + vb)
        numbers.append(number if pick not in (0, 2) else None)
    assert max(len(ln) for ln in a_lines) < 250                # (u8 rows hold offsets up to 254)
    return a_lines, b_lines, np.array(ids, np.int32), np.array(a_caps, np.int32), np.array(b_caps, np.int32), numbers


def csr(lines, dtype, offsets_dtype):
    offsets = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(offsets_dtype)
    return np.frombuffer(b"".join(lines), dtype=np.uint8).astype(dtype), offsets


def pack(ids, caps, dtype):
    rows = (np.concatenate([ids[:, None].astype(np.int64), caps.astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype)
    back = unpack(rows)
    assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    return rows


class Twin:
    """the two batches in one row format, unit width and offset width"""

    def __init__(self, n, fmt="int32", wide=False, off64=False, seed=1):
        a_lines, b_lines, ids, a_caps, b_caps, self.numbers = twins(n, seed)
        dtype, odt = (np.uint16 if wide else np.uint8), (np.uint64 if off64 else np.uint32)
        self.a, self.a_off = csr(a_lines, dtype, odt)
        self.b, self.b_off = csr(b_lines, dtype, odt)
        self.ids, self.a_caps, self.b_caps = ids, a_caps, b_caps
        if fmt == "int32":
            self.a_ids, self.a_rows, self.b_ids, self.b_rows = ids, a_caps, ids, b_caps
        else:
            row_t = np.uint16 if fmt == "u16" else np.uint8
            self.a_ids, self.a_rows, self.b_ids, self.b_rows = pack(ids, a_caps, row_t), None, pack(ids, b_caps, row_t), None
        self.units = "utf-16" if wide else "latin-1"
        self.n = n

    def of(self, k):
        """the numbers of extraction k's lines, sorted"""
        return sorted(v for v, i in zip(self.numbers, self.ids) if i == k and v is not None)

    def a_text(self, index):
        """A's own lines at `index`, as units and offsets"""
        off = self.a_off.astype(np.int64)
        parts = [self.a[off[i]:off[i + 1]] for i in index]
        units = np.concatenate(parts) if parts else np.zeros(0, self.a.dtype)
        return units, np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(self.a_off.dtype)


CASES = [(n, fmt, False, False) for n in SIZES for fmt in ("int32", "u16", "u8")]
CASES += [(n, fmt, True, False) for n in (65, 1000) for fmt in ("int32", "u16", "u8")] + [(1000, "int32", False, True)]
case_ids = ["%d-%s%s%s" % (n, fmt, "-utf16" if wide else "", "-offsets64" if off64 else "") for n, fmt, wide, off64 in CASES]


def middle(values):
    return values[len(values) // 2] if values else 0


def terms_of(gorp, t, op, negate):
    """one integer term per extraction, its number the middle of that extraction's numbers (so that both answers occur)"""
    w = gorp.where_terms([(k, VALUE, op, middle(t.of(k))) for k in range(K)], units=t.units)
    for q in range(w.n):
        assert w.array[q].op >= N.GX_WHERE_INT_EQ
        w.array[q].negate = negate
    return w


@pytest.mark.parametrize("n,fmt,wide,off64", CASES, ids=case_ids)
def test_select_lines_where_every_integer_op_with_negate(n, fmt, wide, off64):
    gorp, _ = handles()
    t = Twin(n, fmt, wide, off64)
    kept_some = dropped_some = False
    for op in ("==", "<", "<=", ">", ">="):
        for negate in (0, 1):
            w = terms_of(gorp, t, op, negate)
            mask = gorp._where_want(w, "matched-by-terms")
            keep = keep_lines(t.b, t.b_off, t.b_ids, t.b_rows, mask, decode_terms(w), K)
            index = selection(t.b, t.b_off, keep)[0]
            units, out_off = t.a_text(index)
            got = gorp.select_lines_where(t.a, t.a_off, t.a_ids, t.a_rows, w, want=mask)
            assert np.array_equal(got[0], index), (op, negate)
            assert got[1].dtype == t.a.dtype and np.array_equal(got[1], units)
            assert got[2].dtype == t.a_off.dtype and np.array_equal(got[2], out_off)
            assert np.array_equal(got[3], t.a_ids[index])
            if fmt == "int32":
                assert np.array_equal(got[4], t.a_caps[index])
            kept_some |= len(index) > 0
            dropped_some |= len(index) < int((t.ids >= 0).sum())
    assert kept_some and dropped_some


def edges_of(values):
    return sorted({values[len(values) * j // 5] for j in range(1, 5)}) if values else []


@pytest.mark.parametrize("n,fmt,wide,off64", CASES, ids=case_ids)
def test_capture_stats_with_edges_and_terms(n, fmt, wide, off64):
    gorp, _ = handles()
    t = Twin(n, fmt, wide, off64)
    measures = gorp.measures([(k, VALUE, edges_of(t.of(k))) for k in range(K)] + [(0, KEY, [3, 6]), (2, VALUE)])   # (a LONG group in the same call)
    for where in ([(1, VALUE, ">=", middle(t.of(1))), (3, VALUE, "<", middle(t.of(3))), (0, KEY, "!=", 5)], []):
        terms = gorp.where_terms(where, units=t.units)
        want = capture_stats(t.b, t.b_off, t.b_ids, t.b_rows, decode_measures(measures), decode_terms(terms), K)
        got = gorp.capture_stats(t.a, t.a_off, t.a_ids, t.a_rows, measures, where=terms)
        same_stats(got, want)
    if n >= 1000:
        assert all(s["numbers"] > 50 and s["not_numbers"] > 10 and s["unset"] > 0 for s in want[:K])   # every class, many times


@pytest.mark.parametrize("n,fmt,wide,off64", CASES, ids=case_ids)
def test_group_lines_group_quantiles_and_top_groups_with_a_value_group(n, fmt, wide, off64):
    gorp, _ = handles()
    t = Twin(n, fmt, wide, off64)
    parts = gorp.group_parts([(k, KEY, VALUE) for k in range(K)])
    dtype = t.a.dtype
    for where in ([], [(2, VALUE, ">", middle(t.of(2))), (0, VALUE, "<=", middle(t.of(0)))]):
        terms = gorp.where_terms(where, units=t.units)
        spec, tspec = group_parts_of(parts), decode_terms(terms)
        same_groups(gorp.group_lines(t.a, t.a_off, t.a_ids, t.a_rows, parts, where=terms, keys="csr"), group_lines(t.b, t.b_off, t.b_ids, t.b_rows, spec, tspec, K), dtype)
        same_quantiles(gorp.group_quantiles(t.a, t.a_off, t.a_ids, t.a_rows, parts, ASKS, where=terms, keys="csr"),
                       group_quantiles(t.b, t.b_off, t.b_ids, t.b_rows, spec, tspec, K, ASKS), ASKS, dtype)
        for by, largest in (("sum", True), ("max", True), ("max", False)):
            got = gorp.top_groups(t.a, t.a_off, t.a_ids, t.a_rows, parts, 5, by=by, largest=largest, where=terms, keys="csr", line_rank=True)
            same_top_groups(got, top_groups(t.b, t.b_off, t.b_ids, t.b_rows, spec, tspec, K, 5, by, largest), 5, largest, dtype)
    # one extraction's keys alone: every number of the key's statistics is in ONE format's unit
    one = gorp.group_parts([(1, KEY, VALUE)])
    same_groups(gorp.group_lines(t.a, t.a_off, t.a_ids, t.a_rows, one, keys="csr"), group_lines(t.b, t.b_off, t.b_ids, t.b_rows, group_parts_of(one), [], K), dtype)


@pytest.mark.parametrize("n,fmt,wide,off64", CASES, ids=case_ids)
def test_top_lines_both_ends_and_capture_quantiles(n, fmt, wide, off64):
    gorp, _ = handles()
    t = Twin(n, fmt, wide, off64)
    for by in ([(k, VALUE) for k in range(K)], [(1, VALUE)], [(3, VALUE), (0, KEY)]):
        parts = gorp.top_parts(by)
        for where in ([], [(1, VALUE, ">=", middle(t.of(1))), (3, VALUE, "!=", middle(t.of(3)))]):
            terms = gorp.where_terms(where, units=t.units)
            spec, tspec = top_parts_of(parts), decode_terms(terms)
            for largest in (True, False):
                w_index, w_values, _, _, w_totals = top_lines(t.b, t.b_off, t.b_ids, t.b_rows, spec, tspec, K, 20, largest)
                index, values, data2, off2, ids2, rows2, totals = gorp.top_lines(t.a, t.a_off, t.a_ids, t.a_rows, parts, 20, largest=largest, where=terms)
                units, out_off = t.a_text(w_index)
                w_totals["units_top"] = len(units)             # (the delivered lines are A's)
                assert totals == w_totals, (totals, w_totals)
                assert index.dtype == np.uint32 and values.dtype == np.int64
                assert np.array_equal(index, w_index) and np.array_equal(values, w_values)
                assert data2.dtype == t.a.dtype and np.array_equal(data2, units) and off2.dtype == t.a_off.dtype and np.array_equal(off2, out_off)
                assert np.array_equal(ids2, t.a_ids[w_index.astype(np.int64)])
                assert (rows2 is None) if fmt != "int32" else np.array_equal(rows2, t.a_caps[w_index.astype(np.int64)])
            want = capture_quantiles(t.b, t.b_off, t.b_ids, t.b_rows, spec, tspec, K, ASKS)
            got = gorp.capture_quantiles(t.a, t.a_off, t.a_ids, t.a_rows, parts, ASKS, where=terms)
            assert got[1] == want[1] and got[0] == want[0], (got, want)


def test_default_path_is_unchanged_bit_for_bit():
    """One LONG-only batch (B), three handles: never given a format, LONG set explicitly, and a format set on a group the calls do not
    name.  Identical bits from all three, and what the restatement says."""
    _, never = handles()
    explicit, elsewhere = construct(), construct()
    for k in range(K):
        explicit.set_number_format(k, "value", "long")
        explicit.set_number_format(k, "key", "long")
        elsewhere.set_number_format(k, "key", "iso8601", 9)
    t = Twin(1000)
    results = []
    for gorp in (never, explicit, elsewhere):
        terms = gorp.where_terms([(k, VALUE, ">=", middle(t.of(k))) for k in range(K)])
        measures = gorp.measures([(k, VALUE, edges_of(t.of(k))) for k in range(K)])
        parts, by = gorp.group_parts([(k, KEY, VALUE) for k in range(K)]), gorp.top_parts([(k, VALUE) for k in range(K)])
        args = (t.b, t.b_off, t.b_ids, t.b_rows)
        sel = gorp.select_lines_where(*args, terms)
        stats = gorp.capture_stats(*args, measures, where=terms)
        groups = gorp.group_lines(*args, parts, keys="csr")
        top = gorp.top_lines(*args, by, 50)
        quant = gorp.capture_quantiles(*args, by, ASKS)
        results.append(repr([[np.asarray(x).tolist() for x in sel], [sorted((k, np.asarray(v).tolist()) for k, v in s.items()) for s in stats],
                             sorted((k, v if isinstance(v, (dict, list)) or v is None else np.asarray(v).tolist()) for k, v in groups.items()),
                             [x if isinstance(x, dict) or x is None else np.asarray(x).tolist() for x in top], quant]))
        if gorp is never:
            same_stats(stats, capture_stats(*args, decode_measures(measures), decode_terms(terms), K))
            same_groups(groups, group_lines(*args, group_parts_of(parts), [], K))
            assert np.array_equal(sel[0], selection(t.b, t.b_off, keep_lines(*args, gorp._where_want(terms, "matched-by-terms"), decode_terms(terms), K))[0])
    assert results[0] == results[1] == results[2]
    # ... and the same batch under the formats is another answer: the twins' values are decimal digits, not stamps
    formatted, _ = handles()
    assert formatted.capture_stats(t.b, t.b_off, t.b_ids, t.b_rows, [(1, VALUE)])[0]["numbers"] == 0


# ---------------------------------------------------------------------------
# end to end: the syslog workload, extracted on the device, `ts` as ISO8601(0)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syslog():
    rules, meta = W.syslog_definition(4)
    gorp = Gorp.construct(rules)
    data, offsets, _ = W.syslog_lines(meta, 2000, seed=11)
    data, offsets = np.asarray(data, np.uint8), np.asarray(offsets, np.uint32)
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids >= 0).sum() > 1900 and (ids < 0).sum() > 5     # the 2 % corrupted lines stay in
    for k in range(4):
        gorp.set_number_format(k, "ts", "iso8601", 0)
    return gorp, data, offsets, ids, caps


def ts_values(data, offsets, ids, caps, k, g=0, kind=NO.ISO8601):
    """per line of extraction k: what the restatement makes of its `ts` (or of group g under `kind`) -- the units of str(number), of `x`,
    or None for an unset group"""
    out = []
    for i in np.flatnonzero(ids == k):
        b, e = int(caps[i, 2 * g]), int(caps[i, 2 * g + 1])
        v = NO.parse(kind, 0, data[int(offsets[i]) + b:int(offsets[i]) + e].tolist()) if b >= 0 else None
        out.append(None if b < 0 else list(b"x" if v is None else b"%d" % v))
    return out


def test_syslog_ts_first_and_last_seen_and_the_lines_since(syslog):
    gorp, data, offsets, ids, caps = syslog
    assert [gorp._extractions[k]._extractorNames[0] for k in range(4)] == ["ts"] * 4
    edges = [parse_number("iso8601", 0, "2026-01-0%dT00:00:00Z" % d) for d in range(2, 10)]
    measures = [("rule%d" % k, "ts", edges) for k in range(4)] + [("rule0", "pid")]
    want = [summarise(ts_values(data, offsets, ids, caps, k), edges) for k in range(4)] + [summarise(ts_values(data, offsets, ids, caps, 0, 2, NO.LONG), [])]
    got = gorp.capture_stats(data, offsets, ids, caps, measures)
    same_stats(got, want)
    first, last = parse_number("iso8601", 0, "2026-01-01T00:00:00Z"), parse_number("iso8601", 0, "2026-01-09T09:00:00Z")
    assert all(first <= s["min"] < s["max"] <= last and s["numbers"] > 400 for s in got[:4]) and sum(s["not_numbers"] for s in got[:4]) > 0
    # the whole-file form: raw text in, the same summary out
    lines = [bytes(data[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(ids))]
    text_stats, counts, n_lines = gorp.text_capture_stats(b"\n".join(lines) + b"\n", measures)
    same_stats(text_stats, want)
    assert n_lines == len(ids) and counts[:4].tolist() == [int((ids == k).sum()) for k in range(4)]
    # the lines since <mid>, the term's number given as a string
    mid = "2026-01-05T05:00:00Z"
    sel = gorp.select_lines_where(data, offsets, ids, caps, [("rule%d" % k, "ts", ">=", mid) for k in range(4)])
    since = parse_number("iso8601", 0, mid)
    keep = np.zeros(len(ids), bool)
    for k in range(4):
        at = np.flatnonzero(ids == k)
        keep[at] = [v is not None and v != list(b"x") and int(bytes(v)) >= since for v in ts_values(data, offsets, ids, caps, k)]
    index, units, out_off = selection(data, offsets, keep)
    assert 600 < len(index) < 1400
    assert np.array_equal(sel[0], index) and np.array_equal(sel[1], units) and np.array_equal(sel[2], out_off)
