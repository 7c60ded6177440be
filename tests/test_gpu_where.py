"""GPU tests of gx_select_lines_where / gx_text_select_where: lines chosen by WHAT they captured.

Expected values come from tests/where_oracle.py -- the value sliced out of the line with the capture offsets, then ==, slices and
re.fullmatch(rb"[+-]?[0-9]+") plus a range check -- and np.flatnonzero / np.cumsum of the kept lines.  The sweeps fabricate ids and
capture rows against handles of K identical, trivial extractions; the end-to-end cases take them from gx_extract_batch.  Everything is
compared exactly."""
import ctypes as C
import random

import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import DefinitionReader, FlattenedExtraction, Gorp, GorpError, lines_to_csr, split_lines
from oracle import oracle as O
from where_oracle import (INT_NUMBERS, INT_OPS, INT_TABLE, LITERAL_LENGTHS, TEXT_OPS, decode_terms, keep_lines, near_miss_cases, outcome, selection,
                          unpack)

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 2048          # gx_scan.hpp: items per workgroup of the scan
SELECT_LDS_BINS = 8192     # gx_device.hpp: beyond 2K + 2 = 8192 bins the want mask stays in global memory
OP_NAME = {N.GX_WHERE_EQ: "==", N.GX_WHERE_PREFIX: "startswith", N.GX_WHERE_SUFFIX: "endswith", N.GX_WHERE_CONTAINS: "contains",
           N.GX_WHERE_INT_EQ: "==", N.GX_WHERE_INT_LT: "<", N.GX_WHERE_INT_LE: "<=", N.GX_WHERE_INT_GT: ">", N.GX_WHERE_INT_GE: ">="}
PUT, GET, OTHER = 0, 1, 2  # workloads.readme3_definition: the extractions' indices; groups timestamp, verb, timeTakenInMsec, path
K3 = 3


def units_of(gorp, data, utf8=None):
    return "utf-16" if data.dtype == np.uint16 else "utf-8" if utf8 else "latin-1"


def check_where(gorp, data, offsets, ids, caps, where, want="matched-by-terms", utf8=None):
    """select_lines_where against the restatement, every output; returns (what the call returned, the kept lines as bool[n])."""
    K = gorp.num_extractions
    w = gorp.where_terms(where, units=units_of(gorp, data, utf8))
    mask = gorp._where_want(w, want)
    keep = keep_lines(data, offsets, ids, caps, mask, decode_terms(w), K)
    index, units, out_off = selection(data, offsets, keep)
    got = gorp.select_lines_where(data, offsets, ids, caps, w, want=mask, utf8=utf8)
    assert np.array_equal(got[0], index)
    assert got[1].dtype == data.dtype and np.array_equal(got[1], units)
    assert got[2].dtype == offsets.dtype and np.array_equal(got[2], out_off)
    if ids.ndim == 2 or caps is not None:
        assert np.array_equal(got[3], ids[index])
    if ids.ndim == 1 and caps is not None:
        assert np.array_equal(got[4], caps[index])
    return got, keep


_handles = {}


def trivial_handle(K, groups=1):
    """K identical extractions `a(.*)...`: a handle for ids and capture rows made up here."""
    if (K, groups) not in _handles:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(groups)]
        _handles[K, groups] = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(K)])
        assert _handles[K, groups].num_extractions == K and _handles[K, groups].max_groups == groups
    return _handles[K, groups]


def csr(lines, dtype=np.uint8, offsets_dtype=np.uint32):
    """lines: sequences of code units"""
    offsets = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(offsets_dtype)
    data = np.array([u for ln in lines for u in ln], dtype=dtype)
    return data, offsets


def with_negate(gorp, spec, units="latin-1"):
    """the terms of spec, and the same with every negate flipped"""
    a, b = gorp.where_terms(spec, units=units), gorp.where_terms(spec, units=units)
    for t in range(b.n):
        b.array[t].negate ^= 1
    return a, b


# ---------------------------------------------------------------------------
# the README definition: GetRequest / PutRequest / OtherRequest, unmatched lines, lines that raise
# ---------------------------------------------------------------------------
def readme_lines(n, seed, tail=".html"):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        verb = rng.choice(["GET"] * 4 + ["PUT"] * 3 + ["POST", "DELETE", "HEAD"])
        ms = rng.choice([rng.randrange(0, 10), rng.randrange(0, 1000), rng.randrange(0, 100000), 500, 499, 7]) if rng.random() < 0.9 else "007"
        path = "/" + rng.choice(["v1/", "v2/", "api/v1/x", "v", ""]) + "".join(rng.choice("abcEL/._-7") for _ in range(rng.randrange(0, 40)))
        path += rng.choice([tail, ".htm", ""])
        line = "[%d]: %s %sms %s" % (rng.randrange(1, 10 ** 9), verb, ms, path)
        r = rng.random()
        if r < 0.08:
            line = line.replace("]: ", "]; ")                       # no extraction matches
        elif r < 0.14:
            line = line + "\x0bq"                                   # the automaton takes VT for \S, the capture regexp does not: the line raises
        elif r < 0.17:
            line = ""
        out.append(line)
    return out


def oracle_for(definition):
    built = [e.build() for e in definition]
    return O.OracleGorp([b[0] for b in built], [b[1] for b in built])


@pytest.fixture(scope="module")
def readme():
    gorp = Gorp.construct(W.readme3_definition())
    lines = readme_lines(2000, seed=3)
    data, offsets = lines_to_csr([ln.encode("latin-1") for ln in lines])
    ids, caps = oracle_for(W.readme3_definition()).extract_batch(data, offsets)
    gids, gcaps = gorp.extract_batch(data, offsets)
    assert np.array_equal(gids, ids) and np.array_equal(gcaps, caps)
    counts = np.bincount(outcome(ids, K3), minlength=2 * K3 + 2)
    assert (counts[:K3 + 1] > 20).all() and counts[K3 + 1:2 * K3 + 1].sum() > 20 and counts[2 * K3 + 1] == 0
    return gorp, data, offsets, ids, caps


THREE = [FlattenedExtraction("ab", [["text", "a"], ["extractor", "x", [["pattern", ".*"]]], ["text", "b"]]),   # "a\rb": the automaton says yes, the regexp no
         FlattenedExtraction("cee", [["text", "c"], ["extractor", "w", [["pattern", "\\w*"]]]]),
         FlattenedExtraction("dee", [["text", "d="], ["extractor", "n", [["pattern", "\\d+"]]], ["pattern", ".*"]])]


def test_no_terms_is_select_lines_bit_for_bit(readme):
    gorp = Gorp.construct(THREE)
    rng = random.Random(5)
    lines = []
    for _ in range(3000):
        body = bytes(rng.choice(b"abcd xyz019=\t") for _ in range(rng.randrange(0, 120)))
        lines.append(rng.choice([b"a" + body + b"b", b"a" + body + b"\r" + body + b"b", b"c" + body, b"d=77" + body, b"", body])[:200])
    data, offsets = lines_to_csr(lines)
    ids, caps = gorp.extract_batch(data, offsets)
    assert len(set(outcome(ids, K3).tolist())) >= 5
    rows16, rows8 = gorp.extract_batch(data, offsets, compact=1)[0], gorp.extract_batch(data, offsets, compact=2)[0]
    for want in ("unmatched", "exceptions", ["ab", "dee"], ["cee", "unmatched", "exceptions"], np.ones(7, np.uint8), np.zeros(7, np.uint8)):
        for id_col, rows in ((ids, caps), (ids, None), (rows16, None), (rows8, None)):
            a = gorp.select_lines(data, offsets, id_col, rows=rows, want=want)
            b = gorp.select_lines_where(data, offsets, id_col, rows, [], want=want)
            assert len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
    # the default want of no terms keeps nothing
    assert len(gorp.select_lines_where(data, offsets, ids, caps, [])[0]) == 0
    # ... and so does a README batch
    gorp, data, offsets, ids, caps = readme
    a, b = gorp.select_lines(data, offsets, ids, rows=caps, want=["GetRequest", "unmatched"]), gorp.select_lines_where(data, offsets, ids, caps, [], want=["GetRequest", "unmatched"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_readme_definition_every_op_and_negate(readme):
    gorp, data, offsets, ids, caps = readme
    singles = [("GetRequest", "timeTakenInMsec", ">=", 500), ("GetRequest", "timeTakenInMsec", ">", 499), ("GetRequest", "timeTakenInMsec", "<", 500),
               ("PutRequest", "timeTakenInMsec", "<=", 7), ("GetRequest", "timeTakenInMsec", "==", 7), ("OtherRequest", "timeTakenInMsec", "!=", 500),
               ("OtherRequest", "verb", "==", "POST"), ("OtherRequest", "verb", "!=", "POST"), ("OtherRequest", "verb", "startswith", "DE"),
               ("OtherRequest", "verb", "endswith", "D"), ("GetRequest", "path", "contains", "/v1/"), ("GetRequest", "path", "not contains", "EL"),
               ("PutRequest", "path", "endswith", ".html"), ("PutRequest", "path", "set"), ("GetRequest", "verb", "unset"), ("GetRequest", "path", "==", "/"),
               ("GetRequest", "path", "startswith", ""), ("GetRequest", "path", "==", "")]
    seen_ops = set()
    for spec in singles:
        for w in with_negate(gorp, [spec]):
            seen_ops.add((w.array[0].op, w.array[0].negate))
            check_where(gorp, data, offsets, ids, caps, w)
    assert seen_ops == {(op, neg) for op in range(10) for neg in (0, 1)}
    # the caller's loop: Long.parseLong(r.asMap().get("timeTakenInMsec")) >= 500
    got, keep = check_where(gorp, data, offsets, ids, caps, [("GetRequest", "timeTakenInMsec", ">=", 500)])
    assert 20 < keep.sum() < (ids == GET).sum() - 20 and (ids[keep] == GET).all()
    for i in np.flatnonzero(ids == GET):
        o = int(offsets[i])
        assert keep[i] == (int(bytes(data[o + caps[i, 4]:o + caps[i, 5]])) >= 500)
    # two terms on one extraction are ANDed
    a = check_where(gorp, data, offsets, ids, caps, [("GetRequest", "timeTakenInMsec", ">=", 100)])[1]
    b = check_where(gorp, data, offsets, ids, caps, [("GetRequest", "path", "contains", "/v1/")])[1]
    both = check_where(gorp, data, offsets, ids, caps, [("GetRequest", "timeTakenInMsec", ">=", 100), ("GetRequest", "path", "contains", "/v1/")])[1]
    assert np.array_equal(both, a & b) and 0 < both.sum() < min(a.sum(), b.sum())
    # terms on two and three extractions at once, given in any order
    spec = [("PutRequest", "path", "startswith", "/v2"), ("GetRequest", "timeTakenInMsec", ">=", 500), ("OtherRequest", "verb", "==", "HEAD"),
            ("PutRequest", "timeTakenInMsec", "<", 1000)]
    keep = check_where(gorp, data, offsets, ids, caps, spec)[1]
    assert all(0 < (keep & (ids == k)).sum() < (ids == k).sum() for k in (PUT, GET, OTHER))
    check_where(gorp, data, offsets, ids, caps, spec[:2])
    # want decides everything that has no terms: the unmatched lines and the exceptions compose with the terms
    keep = check_where(gorp, data, offsets, ids, caps, spec[1:2], want=["GetRequest", "OtherRequest", "unmatched", "exceptions"])[1]
    assert keep[ids == OTHER].all() and keep[ids < 0].all() and not keep[ids == PUT].any() and 0 < keep[ids == GET].sum() < (ids == GET).sum()
    # terms of an extraction that want leaves out change nothing
    keep = check_where(gorp, data, offsets, ids, caps, spec, want="unmatched")[1]
    assert np.array_equal(keep, ids == -1)


def test_selected_batch_extracts_to_the_selected_rows(readme):
    gorp, data, offsets, ids, caps = readme
    (index, sdata, soff, sids, scaps), keep = check_where(gorp, data, offsets, ids, caps, [("GetRequest", "timeTakenInMsec", ">=", 500), ("PutRequest", "path", "endswith", ".html")],
                                                          want=["GetRequest", "PutRequest", "unmatched", "exceptions"])
    again_ids, again_caps = gorp.extract_batch(sdata, soff)
    assert len(index) > 100 and np.array_equal(again_ids, sids) and np.array_equal(again_caps, scaps)


# ---------------------------------------------------------------------------
# value lengths x literal lengths x source misalignment
# ---------------------------------------------------------------------------
_sweep = {}


def sweep_batch():
    """One extraction per (literal length, text op), each with one term; a line per case of near_miss_cases, its id the extraction of
    its literal and op, its capture row the case's offsets."""
    if not _sweep:
        cases = near_miss_cases(sorted(set(range(0, 41)) | {63, 64, 65, 254, 255, 256, 300}))
        cases.sort(key=lambda c: c[4] == len(c[2]))          # (the last line's capture ends with the line)
        lits = {}
        for op, _, buf, b, e, lit, _, _ in cases:
            lits.setdefault(len(lit), lit)
            assert lits[len(lit)] == lit
        ext = {(ln, op): k for k, (ln, op) in enumerate((ln, op) for ln in LITERAL_LENGTHS for op in TEXT_OPS)}
        spec = [(k, 0, OP_NAME[op], bytes(lits[ln])) for (ln, op), k in ext.items()]
        data, offsets = csr([c[2] for c in cases])
        ids = np.array([ext[len(c[5]), c[0]] for c in cases], np.int32)
        caps = np.array([[c[3], c[4]] for c in cases], np.int32)
        _sweep.update(spec=spec, data=data, offsets=offsets, ids=ids, caps=caps, K=len(ext))
    return _sweep


@pytest.mark.parametrize("mis", range(16))
def test_value_and_literal_lengths_at_every_misalignment(mis):
    import torch
    s = sweep_batch()
    gorp = trivial_handle(s["K"])
    data, offsets, ids, caps = s["data"], s["offsets"], s["ids"], s["caps"]
    n = len(ids)
    assert n > 5000 and caps[-1, 1] == offsets[-1] - offsets[-2]            # the last capture ends at the buffer's last byte
    w = gorp.where_terms(s["spec"])
    mask = gorp._where_want(w, "matched-by-terms")
    keep = keep_lines(data, offsets, ids, caps, mask, decode_terms(w), s["K"])
    assert 0.1 * n < keep.sum() < 0.9 * n
    index, units, out_off = selection(data, offsets, keep)
    src = torch.empty(mis + len(data), dtype=torch.uint8, device="cuda")     # sized exactly: the batch ends where the tensor ends
    src[mis:] = torch.from_numpy(data).cuda()
    d_off, d_ids, d_caps = torch.from_numpy(offsets.view(np.int32)).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(caps).cuda()
    args = (src.data_ptr() + mis, d_off.data_ptr(), n, d_ids.data_ptr(), d_caps.data_ptr(), mask, w)
    assert gorp.select_lines_where_device(*args) == (len(index), len(units))
    d_index = torch.full((len(index) + 2,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    d_out = torch.full((len(units) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert gorp.select_lines_where_device(*args, out_index_ptr=d_index.data_ptr() + 4, out_data_ptr=d_out.data_ptr(), cap_lines=len(index),
                                          out_bytes_cap=len(units)) == (len(index), len(units))
    oi, out = d_index.cpu().numpy(), d_out.cpu().numpy()
    assert oi[0] == oi[-1] == 0x7FFFFFFF and np.array_equal(oi[1:-1].view(np.uint32), index)
    assert np.array_equal(out[:len(units)], units) and (out[len(units):] == 0xA5).all()


# ---------------------------------------------------------------------------
# integers
# ---------------------------------------------------------------------------
def test_the_integer_table_through_the_kernel():
    terms = [(op, num, neg) for op in INT_OPS for num in INT_NUMBERS for neg in (0, 1)]
    gorp = trivial_handle(len(terms))
    w = gorp.where_terms([(k, 0, OP_NAME[op], num) for k, (op, num, neg) in enumerate(terms)])
    for k, (op, num, neg) in enumerate(terms):
        assert w.array[k].op == op
        w.array[k].negate = neg
    lines, ids, caps = [], [], []
    for k in range(len(terms)):
        for v in INT_TABLE:
            lines += [v, b"x" + v + b"9"]                     # the value alone, and between units that would change the number
            caps += [[0, len(v)], [1, 1 + len(v)]]
            ids += [k, k]
    data, offsets = csr(lines)
    keep = check_where(gorp, data, offsets, np.array(ids, np.int32), np.array(caps, np.int32), w)[1]
    assert 0.3 * len(ids) < keep.sum() < 0.7 * len(ids)


# ---------------------------------------------------------------------------
# row formats, offset widths, unset groups, pairs that name no value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offsets_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("fmt", ["int32", "u16", "u8"])
def test_row_formats_unset_groups_and_invalid_pairs(readme, fmt, offsets_dtype):
    gorp, data, offsets, ids, caps = readme
    offsets = offsets.astype(offsets_dtype)
    lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
    assert lens.max() < 250                                  # (u8 rows hold every offset)
    rng = np.random.default_rng(17)
    caps = caps.copy()
    get = np.flatnonzero(ids == GET)[:-1]                    # (not the batch's last line: "beyond the line" stays inside the buffer)
    kinds = rng.integers(0, 6, len(get))
    for i, kind in zip(get, kinds):
        if kind == 1:
            caps[i, 4:6] = -1                                # the group is unset
        elif kind == 2:
            caps[i, 5] = lens[i] + 1                         # end beyond the line's end
        elif kind == 3:
            caps[i, 4], caps[i, 5] = caps[i, 5], caps[i, 4] - 1   # end < begin
        elif kind == 4:
            caps[i, 4] = -1                                  # begin < 0 <= end
    if fmt == "int32":
        id_col, rows = ids, caps
    else:
        dtype = np.uint16 if fmt == "u16" else np.uint8
        id_col, rows = (np.concatenate([ids[:, None].astype(np.int64), caps.astype(np.int64)], axis=1) & np.iinfo(dtype).max).astype(dtype), None
        back = unpack(id_col)
        assert np.array_equal(back[0], ids) and np.array_equal(back[1], caps)
    damaged = np.zeros(len(ids), bool)
    damaged[get[kinds >= 1][kinds[kinds >= 1] <= 4]] = True
    for spec, expect in (([("GetRequest", "timeTakenInMsec", "set")], "sound"), ([("GetRequest", "timeTakenInMsec", "unset")], "damaged"),
                         ([("GetRequest", "timeTakenInMsec", ">=", 0)], "sound"), ([("GetRequest", "timeTakenInMsec", "!=", -1)], "all"),
                         ([("GetRequest", "timeTakenInMsec", "not contains", "zz")], "all"), ([("GetRequest", "timeTakenInMsec", "startswith", "")], "sound"),
                         ([("GetRequest", "timeTakenInMsec", ">=", 500), ("GetRequest", "path", "contains", "v")], None)):
        keep = check_where(gorp, data, offsets, id_col, rows, spec, want=["GetRequest", "unmatched"])[1]
        is_get = ids == GET
        if expect == "sound":
            assert np.array_equal(keep[is_get], ~damaged[is_get])
        elif expect == "damaged":
            assert np.array_equal(keep[is_get], damaged[is_get])
        elif expect == "all":
            assert keep[is_get].all()
        assert keep[ids == -1].all() and not keep[(ids != GET) & (ids != -1)].any()
    assert 100 < damaged.sum() < len(get) - 100


# ---------------------------------------------------------------------------
# code units: UTF-16, UTF-8 bytes
# ---------------------------------------------------------------------------
def test_utf16_units_literals_above_0xff_and_digits():
    gorp = Gorp.construct(W.readme3_definition())
    rng = random.Random(8)
    lines = []
    for ln in readme_lines(1500, seed=9):
        lines.append(ln.replace("/v1/", rng.choice(["/v1/", "/Ж€/", "/Ж/"])))
    units = [np.frombuffer(s.encode("utf-16-le"), dtype=np.uint16) for s in lines]
    data, offsets = csr(units, dtype=np.uint16)
    assert (data > 0xFF).any()
    ids, caps = gorp.extract_batch(data, offsets)
    assert (ids == GET).sum() > 300
    for spec in ([("GetRequest", "path", "contains", "Ж€")], [("GetRequest", "path", "startswith", "/Ж")], [("GetRequest", "path", "not contains", "€")],
                 [("GetRequest", "timeTakenInMsec", ">=", 500)], [("GetRequest", "timeTakenInMsec", ">=", 500), ("GetRequest", "path", "contains", "/Ж/")],
                 [("OtherRequest", "verb", "==", "POST")]):
        keep = check_where(gorp, data, offsets, ids, caps, spec)[1]
        assert 0 < keep.sum() < (ids >= 0).sum()
    # a unit whose low byte is the literal's is another unit; U+FF11 is a digit to Character.digit and none here
    gorp = trivial_handle(2)
    lines = [[0x31], [0xFF11], [0x31, 0xFF11], [0x31, 0x32], [0x131, 0x32], [0x2D, 0x37], [0x2D, 0xFF17], [0x416], [0x16], [0x0416, 0x31]]
    data, offsets = csr(lines * 2, dtype=np.uint16)
    ids = np.array([0] * len(lines) + [1] * len(lines), np.int32)
    caps = np.array([[0, len(ln)] for ln in lines * 2], np.int32)
    keep = check_where(gorp, data, offsets, ids, caps, [(0, 0, ">=", -100), (1, 0, "startswith", "Ж")])[1]
    assert keep.tolist() == [True, False, False, True, False, True, False, False, False, False] + [False] * 7 + [True, False, True]


def test_utf8_bytes_rows_and_a_literal_that_is_not_ascii():
    gorp = Gorp.construct(W.readme3_definition())
    rng = random.Random(12)
    lines = [ln.replace("/v1/", rng.choice(["/v1/", "/café/", "/cafe/", "/café"])) for ln in readme_lines(1500, seed=13)]
    data, offsets = lines_to_csr([ln.encode("utf-8") for ln in lines])
    assert (data >= 0x80).any()
    ids, caps = gorp.extract_batch(data, offsets, utf8="bytes")
    for spec in ([("GetRequest", "path", "contains", "café")], [("GetRequest", "path", "contains", "é/")], [("PutRequest", "path", "not contains", "é")],
                 [("GetRequest", "path", "contains", "café"), ("GetRequest", "timeTakenInMsec", "<", 500)]):
        keep = check_where(gorp, data, offsets, ids, caps, spec, utf8="bytes")[1]
        assert 0 < keep.sum() < (ids >= 0).sum()
    for i in np.flatnonzero(check_where(gorp, data, offsets, ids, caps, [("GetRequest", "path", "contains", "café")], utf8="bytes")[1]):
        assert "café" in lines[i]
    with pytest.raises(ValueError):
        gorp.select_lines_where(data, offsets, ids, caps, [], utf8="units")


def test_lines_keep_their_terminators_and_a_suffix_ends_with_the_line():
    gorp = Gorp.construct(W.readme3_definition())
    rng = random.Random(9)
    lines = [ln for ln in readme_lines(1500, seed=4) if ln and "\x0b" not in ln]     # (an empty line between "\r" and "\n" would be none)
    text = b"".join(ln.encode("latin-1") + rng.choice([b"\n", b"\r\n", b"\r"]) for ln in lines) + b"[12]: GET 5ms /last/line/without/one.html"
    data = np.frombuffer(text, dtype=np.uint8)
    offsets, _ = split_lines(text)
    assert len(offsets) - 1 == len(lines) + 1
    ids, caps = gorp.extract_batch(data, offsets, strip_eol=True)
    assert ids[-1] == GET and caps[-1, 7] == offsets[-1] - offsets[-2]
    for spec in ([("GetRequest", "path", "endswith", ".html")], [("GetRequest", "path", "endswith", "l")], [("PutRequest", "path", "endswith", ".htm")],
                 [("GetRequest", "path", "endswith", ".html\n")], [("GetRequest", "path", "endswith", "\n")]):
        got, keep = check_where(gorp, data, offsets, ids, caps, spec)
        index, out = got[0], got[1]
        assert out.tobytes() == b"".join(text[offsets[i]:offsets[i + 1]] for i in index)
        assert (keep.sum() == 0) == ("\n" in spec[0][3])
        if keep.sum():
            assert keep[-1] == (spec[0][0] == "GetRequest") and keep.sum() < (ids == (GET if spec[0][0] == "GetRequest" else PUT)).sum()


# ---------------------------------------------------------------------------
# sizes: lines, extractions, terms
# ---------------------------------------------------------------------------
def made_up_batch(K, n, seed, with_terms):
    """n short lines of digits with ids drawn from the extractions in with_terms, a few others, no match and exceptions."""
    rng = np.random.default_rng(seed)
    pool = np.array(sorted(set(with_terms) | {0, K // 2, K - 1}) + [-1, -2, -1 - K], np.int32)
    ids = rng.choice(pool, n)
    lens = rng.integers(0, 7, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    data = rng.integers(0x30, 0x3A, int(offsets[-1]), dtype=np.uint8)
    caps = np.stack([np.zeros(n, np.int64), lens], axis=1).astype(np.int32)
    caps[rng.random(n) < 0.1] = -1
    return data, offsets, ids, caps


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_line_counts_around_wave_workgroup_and_scan_boundaries(n):
    gorp = trivial_handle(3)
    data, offsets, ids, caps = made_up_batch(3, n, seed=n, with_terms=[0, 2])
    spec = [(0, 0, ">=", 500), (2, 0, "contains", "7")]
    for want in ("matched-by-terms", [0, 1, 2, "unmatched"], ["exceptions", 2]):
        keep = check_where(gorp, data, offsets, ids, caps, spec, want=want)[1]
    assert n < 64 or 0 < keep.sum() < n


@pytest.mark.parametrize("K", [1, 31, 32, 2048, SELECT_LDS_BINS // 2 + 1])
def test_extraction_counts_first_last_and_64_terms(K):
    gorp = trivial_handle(K)
    assert (2 * K + 2 > SELECT_LDS_BINS) == (K > 4095)
    n = 6000
    # terms on the first and on the last extraction
    data, offsets, ids, caps = made_up_batch(K, n, seed=K, with_terms=[0, K - 1])
    spec = [(0, 0, ">=", 500), (K - 1, 0, "contains", "7")]
    keep = check_where(gorp, data, offsets, ids, caps, spec, want=[0, K // 2, K - 1, "unmatched"])[1]
    assert 0 < keep[ids == 0].sum() < (ids == 0).sum() and 0 < keep[ids == K - 1].sum() < (ids == K - 1).sum() and keep[ids == -1].all()
    assert not keep[ids < -1].any()
    # 64 terms at once, over as many extractions as there are (up to 64 of them, the first and the last among them)
    ext = sorted(set(np.linspace(0, K - 1, min(K, 64)).astype(int).tolist()))
    ops = [lambda j: (">=", 10 * j), lambda j: ("contains", str(j % 10)), lambda j: ("<", 900000 - j), lambda j: ("not contains", "%d%d" % (j % 10, j % 7)),
           lambda j: ("startswith", ""), lambda j: ("set", None)]
    order = np.random.default_rng(K).permutation(64)
    spec = [(ext[int(j) % len(ext)], 0) + ops[int(j) % len(ops)](int(j)) for j in order]
    assert len(spec) == 64
    data, offsets, ids, caps = made_up_batch(K, n, seed=K + 1, with_terms=ext)
    keep = check_where(gorp, data, offsets, ids, caps, spec)[1]
    assert K == 1 or 0 < keep.sum() < np.isin(ids, ext).sum()
    check_where(gorp, data, offsets, ids, caps, spec, want=np.ones(2 * K + 1, np.uint8))
    with pytest.raises(GorpError) as ei:
        gorp.select_lines_where(data, offsets, ids, caps, spec + [(0, 0, "set")])
    assert ei.value.code == N.GX_E_LIMIT


# ---------------------------------------------------------------------------
# capacity, stream order
# ---------------------------------------------------------------------------
def test_size_query_equals_run_and_a_capacity_too_small_writes_nothing(readme):
    import torch
    gorp, data, offsets, ids, caps = readme
    w = gorp.where_terms([("GetRequest", "timeTakenInMsec", ">=", 500), ("PutRequest", "path", "contains", "v")])
    mask = gorp.want_mask(["GetRequest", "PutRequest", "unmatched", "exceptions"])
    keep = keep_lines(data, offsets, ids, caps, mask, decode_terms(w), K3)
    index, units, out_off = selection(data, offsets, keep)
    k, nbytes = len(index), len(units)
    d = {name: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in
         (("data", data.copy()), ("off", offsets), ("ids", ids), ("caps", caps))}
    inputs = (d["data"].data_ptr(), d["off"].data_ptr(), len(ids), d["ids"].data_ptr(), d["caps"].data_ptr(), mask, w)
    assert gorp.select_lines_where_device(*inputs) == (k, nbytes)                      # the size query
    POISON = 0x5A
    outs = {"out_index_ptr": torch.full((4 * k,), POISON, dtype=torch.uint8, device="cuda"), "out_data_ptr": torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda"),
            "out_offsets_ptr": torch.full((4 * (k + 1),), POISON, dtype=torch.uint8, device="cuda"), "out_ids_ptr": torch.full((4 * k,), POISON, dtype=torch.uint8, device="cuda"),
            "out_caps_ptr": torch.full((4 * k * caps.shape[1],), POISON, dtype=torch.uint8, device="cuda")}
    ptrs = {name: t.data_ptr() for name, t in outs.items()}
    L = N.lib()
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    for cap_lines, cap_bytes in ((k - 1, nbytes), (k, nbytes - 1), (0, 0)):
        sizes = (C.c_uint64(0), C.c_uint64(0))
        rc = L.gx_select_lines_where(gorp._h.ptr, *inputs[:5], mask.ctypes.data, w.array, w.n, ptrs["out_index_ptr"], ptrs["out_data_ptr"], ptrs["out_offsets_ptr"],
                                     ptrs["out_ids_ptr"], ptrs["out_caps_ptr"], cap_lines, cap_bytes, C.byref(sizes[0]), C.byref(sizes[1]), C.byref(o))
        assert rc == N.GX_E_LIMIT and "smaller than" in N.last_error()
        assert (sizes[0].value, sizes[1].value) == (k, nbytes)
        for t in outs.values():
            assert bool((t == POISON).all())
    assert gorp.select_lines_where_device(*inputs, cap_lines=k, out_bytes_cap=nbytes, **ptrs) == (k, nbytes)
    assert np.array_equal(outs["out_data_ptr"].cpu().numpy(), units)
    assert np.array_equal(outs["out_index_ptr"].cpu().numpy().view(np.uint32), index)
    assert np.array_equal(outs["out_offsets_ptr"].cpu().numpy().view(np.uint32), out_off)
    assert np.array_equal(outs["out_ids_ptr"].cpu().numpy().view(np.int32), ids[index])
    assert np.array_equal(outs["out_caps_ptr"].cpu().numpy().view(np.int32).reshape(k, -1), caps[index])
    # dense ids and terms without capture rows: refused on a handle with a device too
    with pytest.raises(GorpError) as ei:
        gorp.select_lines_where_device(inputs[0], inputs[1], inputs[2], inputs[3], None, mask, w)
    assert ei.value.code == N.GX_E_ARG


def test_the_call_follows_a_no_sync_batch_on_its_stream():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 60000, 200
    data, offsets, cat = W.readme3_lines(n, seed=77, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    width = 1 + 2 * gorp.max_groups
    rows = torch.full((n, width), 0x55, dtype=torch.uint8, device="cuda")       # ids nobody wrote: outcome 2K + 1
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    w = gorp.where_terms([("GetRequest", "timeTakenInMsec", ">=", 500)])
    with torch.cuda.stream(stream):
        gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, None, rows.data_ptr(), stream=stream.cuda_stream, no_sync=True, compact=2,
                                  line_bytes_hint=L)
        k, nbytes = gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, "matched-by-terms", w, compact=2,
                                                   stream=stream.cuda_stream)
        index = torch.empty(k, dtype=torch.int32, device="cuda")
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, "matched-by-terms", w, out_index_ptr=index.data_ptr(),
                                       out_data_ptr=out.data_ptr(), cap_lines=k, out_bytes_cap=nbytes, compact=2, stream=stream.cuda_stream, no_sync=True)
        # (the copy pass may still be reading the handle's workspace: the next call waits for it)
        k2, _ = gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, rows.data_ptr(), None, "matched-by-terms",
                                               [("PutRequest", "timeTakenInMsec", "<", 500)], compact=2, stream=stream.cuda_stream)
    stream.synchronize()
    h_rows, h_data, h_off = rows.cpu().numpy(), data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(unpack(h_rows)[0], cat.cpu().numpy().astype(np.int32))
    keep = keep_lines(h_data, h_off, h_rows, None, gorp.want_mask("GetRequest"), decode_terms(w), K3)
    assert k == keep.sum() > 1000 and nbytes == k * L and keep.sum() < (unpack(h_rows)[0] == GET).sum() - 1000
    assert np.array_equal(index.cpu().numpy().view(np.uint32), np.flatnonzero(keep))
    assert np.array_equal(out.cpu().numpy(), h_data.reshape(n, L)[keep].reshape(-1))
    keep2 = keep_lines(h_data, h_off, h_rows, None, gorp.want_mask("PutRequest"), decode_terms(gorp.where_terms([("PutRequest", "timeTakenInMsec", "<", 500)])), K3)
    assert k2 == keep2.sum() > 1000


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------
def test_text_select_where_is_split_extract_select():
    gorp = DefinitionReader.reader(W.README3_DEFINITION_TEXT).read()
    rng = random.Random(6)
    for utf8 in (False, True):
        lines = readme_lines(3000, seed=21)
        if utf8:
            lines = [ln.replace("/v1/", rng.choice(["/v1/", "/café/", "/Ж€/"])) for ln in lines]
        raw = [ln.encode("utf-8" if utf8 else "latin-1") for ln in lines]
        text = b"".join(ln + rng.choice([b"\n", b"\n", b"\r\n"]) for ln in raw) + b"[123456789]: GET 777ms /tail"
        data = np.frombuffer(text, dtype=np.uint8)
        offsets, _ = split_lines(text)
        ids, caps = gorp.extract_batch(data, offsets, strip_eol=True, utf8="bytes" if utf8 else None)
        counts = gorp.count_outcomes(ids)
        specs = [[("GetRequest", "timeTakenInMsec", ">=", 500)], [("GetRequest", "timeTakenInMsec", ">=", 500), ("PutRequest", "path", "contains", "/v2/")],
                 [("OtherRequest", "verb", "!=", "POST")]]
        if utf8:
            specs += [[("GetRequest", "path", "contains", "café")], [("GetRequest", "path", "contains", "Ж€"), ("GetRequest", "timeTakenInMsec", "<", 500)]]
        for spec in specs:
            for want in ("matched-by-terms", ["GetRequest", "unmatched", "exceptions"]):
                (index, out, _, _, _), keep = check_where(gorp, data, offsets, ids, caps, spec, want=want, utf8="bytes" if utf8 else None)
                got, got_counts, n_lines = gorp.text_select_where(text, spec, want=want, utf8=utf8)
                assert got == out.tobytes() and n_lines == len(lines) + 1 and np.array_equal(got_counts, counts)
                assert 0 < len(index) < n_lines
        assert check_where(gorp, data, offsets, ids, caps, specs[0], utf8="bytes" if utf8 else None)[1][-1]       # the tail: 777 >= 500
        # no terms: gx_text_select
        for want in (("unmatched", "exceptions"), "GetRequest", ["PutRequest", "OtherRequest", "unmatched"]):
            a, b = gorp.text_select(text, want, utf8=utf8), gorp.text_select_where(text, [], want=want, utf8=utf8)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert gorp.text_select_where(b"", [("GetRequest", "path", "set")])[0] == b""


# ---------------------------------------------------------------------------
# a batch that lives on the device
# ---------------------------------------------------------------------------
def test_200k_lines_on_the_device():
    import torch
    gorp = Gorp.construct(W.readme3_definition())
    n, L = 200000, 200
    data, offsets, cat = W.readme3_lines(n, seed=12, device="cuda")
    d_off = offsets.to(torch.int64).to(torch.int32)
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    caps = torch.empty((n, 2 * gorp.max_groups), dtype=torch.int32, device="cuda")
    gorp.extract_batch_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
    assert torch.equal(ids, cat.to(torch.int32))
    h_data, h_off, h_ids, h_caps = data.cpu().numpy(), d_off.cpu().numpy().view(np.uint32), ids.cpu().numpy(), caps.cpu().numpy()
    for spec, want in (([("GetRequest", "timeTakenInMsec", ">=", 500)], "matched-by-terms"),
                       ([("OtherRequest", "verb", "==", "POST"), ("GetRequest", "path", "contains", "a/")], ["GetRequest", "OtherRequest", "unmatched"])):
        w = gorp.where_terms(spec)
        mask = gorp._where_want(w, want)
        keep = keep_lines(h_data, h_off, h_ids, h_caps, mask, decode_terms(w), K3)
        k = int(keep.sum())
        assert 5000 < k < n - 10000
        assert gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), mask, w) == (k, k * L)
        out = torch.empty(k * L, dtype=torch.uint8, device="cuda")
        o_index = torch.empty(k, dtype=torch.int32, device="cuda")
        o_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        o_ids = torch.empty(k, dtype=torch.int32, device="cuda")
        o_caps = torch.empty((k, caps.shape[1]), dtype=torch.int32, device="cuda")
        gorp.select_lines_where_device(data.data_ptr(), d_off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), mask, w, out_index_ptr=o_index.data_ptr(),
                                       out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(),
                                       out_caps_ptr=o_caps.data_ptr(), cap_lines=k, out_bytes_cap=k * L)
        t_keep = torch.from_numpy(keep).cuda()
        assert np.array_equal(o_index.cpu().numpy().view(np.uint32), np.flatnonzero(keep))
        assert torch.equal(out, data.view(n, L)[t_keep].reshape(-1))
        assert torch.equal(o_off, (torch.arange(k + 1, device="cuda") * L).to(torch.int32))
        assert torch.equal(o_ids, ids[t_keep]) and torch.equal(o_caps, caps[t_keep])


# ---------------------------------------------------------------------------
# the whole-file call from host buffers and from device pointers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_text_form_from_host_buffers_and_device_pointers(n):
    from twin_buffers import twins
    gorp = Gorp.construct(W.readme3_definition())
    lines = ["[%d]: %s %dms /p/%d" % (i, ("GET", "PUT", "POST")[i % 3], 10 * i, i % 7) for i in range(n)]
    if n > 9:
        lines[5], lines[9] = "", "nothing here"
    text = np.frombuffer("".join(l + "\n" for l in lines).encode(), np.uint8)
    text16 = np.zeros((text.size + 15) // 16 * 16 + 16, np.uint8)       # (a device text is 16-byte aligned: torch's allocations are)
    text16[:text.size] = text
    kept = [l for i, l in enumerate(lines) if i % 3 == 0 and 10 * i >= 300 and i != 9]
    for where, want, expect in (([("GetRequest", "timeTakenInMsec", ">=", 300)], "matched-by-terms", "".join(l + "\n" for l in kept).encode()),
                                ([], ("unmatched", "exceptions"), b"\nnothing here\n" if n > 9 else b"")):
        def size_query(b, device_pointers):
            size, counts, n_lines = gorp.text_select_where_device(b.put(text16), text.size, want, where, None, 0, device_pointers=device_pointers)
            return size, counts.tolist(), n_lines
        (size, counts, n_lines), _ = twins(size_query)
        assert size == len(expect) and n_lines == n and sum(counts) == n

        def call(b, device_pointers):
            got, c, nl = gorp.text_select_where_device(b.put(text16), text.size, want, where, b.room("out", size), size, device_pointers=device_pointers)
            return got, c.tolist(), nl
        (got, counts2, _), rooms = twins(call)
        assert got == size and counts2 == counts and rooms["out"][:size] == expect
