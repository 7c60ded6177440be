"""GPU tests of where the reductions built on gx_group_lines, and gx_bucket_lines, put their outputs: host arrays, which the library
stages in device twins and copies back, and device pointers, which the kernels write themselves, must hold the same bytes -- also in the
states where no kernel writes an output and the host layer fills it in ("no keys", "no lines", "no cells").

Seven verbs -- gx_group_lines, gx_group_quantiles, gx_lines_by_key, gx_group_pairs, gx_group_series, gx_top_groups, gx_bucket_lines --
on five batches of at most three lines, fabricated against a handle of one trivial extraction with three groups (group 0 the key, group 1
the number or the second, group 2 the value):
  (a) no lines
  (b) three lines and no parts
  (c) three lines whose key and number are unset on every line: the build runs and finds no key, no bucket
  (d) three keyed lines with nothing in the second table: no line has a number (no cells), a second (no pairs), and min_lines is above
      every key's count (no kept lines)
  (e) three ordinary lines with two keys
Each batch runs once with host arrays and once with device pointers on the null stream, every output requested, every output buffer 0xAB
before the call and one element longer than the totals of a size query say it must be.  The totals are the same, the bytes are the same,
and nothing lies beyond the written part; in (e) each output requested alone holds the bytes it holds when all are requested."""
import numpy as np
import pytest

from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp
from series_oracle import batch

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
POISON = 0xAB
Q = [(1, 2), (1, 1)]
SLOTS = 6                                                                                     # 2 x the handle's three groups

_handle = []


def handle():
    if not _handle:
        pieces = [["text", "a"]] + [["extractor", "v%d" % g, [["pattern", ".*"]]] for g in range(3)]
        _handle.append(Gorp.construct([FlattenedExtraction("r0", pieces)]))
        assert _handle[0].num_extractions == 1 and _handle[0].max_groups == 3
    return _handle[0]


BATCHES = {
    "a": batch([], []),
    "b": batch([b"x", b"y", b"x"], [5, 7, 5], values=[1, 2, 3]),
    "c": batch([None] * 3, [None] * 3, values=[1, 2, 3]),
    "d": batch([b"x", b"y", b"x"], [None] * 3, values=[1, 2, 3]),
    "e": batch([b"x", b"y", b"x"], [5, 7, 5], values=[1, 2, 3]),
}

# an output: (the wrapper's keyword without "_ptr", bytes per element, elements written as the totals t and the number of lines n say)
KEYS = [("key_units", 1, lambda t, n: t["key_units"]), ("key_offsets", 4, lambda t, n: t["n_keys"] + 1), ("key_first_line", 4, lambda t, n: t["n_keys"]),
        ("key_lines", 8, lambda t, n: t["n_keys"]), ("key_stats", 64, lambda t, n: t["n_keys"]), ("line_key", 4, lambda t, n: n)]
# a verb: its parts, its call, its outputs; then which of them hold one 0 when nothing is found, and which a NONE per line
VERBS = {
    "group_lines": ([(0, 0, 2)], lambda g, a, p, kw: g.group_lines_device(*a, p, key_units_cap=64, max_keys=3, **kw), KEYS, ["key_offsets"], ["line_key"]),
    "group_quantiles": ([(0, 0, 2)], lambda g, a, p, kw: g.group_quantiles_device(*a, p, Q, key_units_cap=64, max_keys=3, **kw),
                        KEYS + [("key_quantiles", 32, lambda t, n: t["n_keys"] * len(Q))], ["key_offsets"], ["line_key"]),
    "lines_by_key": ([(0, 0, 2)], lambda g, a, p, kw: g.lines_by_key_device(*a, p, key_units_cap=64, max_keys=3, cap_lines=3, out_bytes_cap=64, **kw),
                     KEYS + [("out_index", 4, lambda t, n: t["lines_out"]), ("out_data", 1, lambda t, n: t["units_out"]), ("out_offsets", 4, lambda t, n: t["lines_out"] + 1),
                             ("out_ids", 4, lambda t, n: t["lines_out"]), ("out_caps", 4 * SLOTS, lambda t, n: t["lines_out"]),
                             ("key_out_lines", 8, lambda t, n: t["n_keys"] + 1), ("key_out_units", 8, lambda t, n: t["n_keys"] + 1)],
                     ["key_offsets", "out_offsets", "key_out_lines", "key_out_units"], ["line_key"]),
    "group_pairs": ([(0, 0, 1, 2)], lambda g, a, p, kw: g.group_pairs_device(*a, p, key_units_cap=64, max_keys=3, pair_units_cap=64, max_pairs=3, **kw),
                    KEYS + [("pair_units", 1, lambda t, n: t["pair_units"]), ("pair_offsets", 4, lambda t, n: t["n_pairs"] + 1), ("pair_key", 4, lambda t, n: t["n_pairs"]),
                            ("pair_first_line", 4, lambda t, n: t["n_pairs"]), ("pair_lines", 8, lambda t, n: t["n_pairs"]), ("key_pairs", 8, lambda t, n: t["n_keys"]),
                            ("line_pair", 4, lambda t, n: n)],
                    ["key_offsets", "pair_offsets"], ["line_key", "line_pair"]),
    "group_series": ([(0, 0, 1, 2)], lambda g, a, p, kw: g.group_series_device(*a, p, 1, key_units_cap=64, max_keys=3, max_cells=3, max_buckets=3, **kw),
                     KEYS + [("bucket_number", 8, lambda t, n: t["n_buckets"]), ("cell_key", 4, lambda t, n: t["n_cells"]), ("cell_bucket", 4, lambda t, n: t["n_cells"]),
                             ("cell_first_line", 4, lambda t, n: t["n_cells"]), ("cell_lines", 8, lambda t, n: t["n_cells"]), ("cell_stats", 64, lambda t, n: t["n_cells"]),
                             ("key_cell_begin", 8, lambda t, n: t["n_keys"] + 1), ("line_cell", 4, lambda t, n: n)],
                     ["key_offsets", "key_cell_begin"], ["line_key", "line_cell"]),
    "top_groups": ([(0, 0, 2)], lambda g, a, p, kw: g.top_groups_device(*a, p, 3, key_units_cap=64, cap_keys=3, max_keys=3, **kw),
                   [("key_units", 1, lambda t, n: t["units_top"]), ("key_offsets", 4, lambda t, n: t["n_top"] + 1), ("key_number", 4, lambda t, n: t["n_top"]),
                    ("key_first_line", 4, lambda t, n: t["n_top"]), ("key_lines", 8, lambda t, n: t["n_top"]), ("key_stats", 64, lambda t, n: t["n_top"]),
                    ("line_rank", 4, lambda t, n: n)],
                   ["key_offsets"], ["line_rank"]),
    "bucket_lines": ([(0, 1, 2)], lambda g, a, p, kw: g.bucket_lines_device(*a, p, 1, max_buckets=3, **kw),
                     [("bucket_number", 8, lambda t, n: t["n_buckets"]), ("bucket_first_line", 4, lambda t, n: t["n_buckets"]), ("bucket_lines", 8, lambda t, n: t["n_buckets"]),
                      ("bucket_stats", 64, lambda t, n: t["n_buckets"]), ("line_bucket", 4, lambda t, n: n)],
                     [], ["line_bucket"]),
}
FOUND = {"group_lines": "n_keys", "group_quantiles": "n_keys", "lines_by_key": "lines_out", "group_pairs": "n_pairs", "group_series": "n_cells", "top_groups": "n_top",
         "bucket_lines": "n_buckets"}


def flat(totals):
    """a verb's totals with the group's beside its own (gx_top_groups nests them only)"""
    return dict(totals.get("group", {}), **totals)


class Runner:
    """One verb on one batch: the inputs in host and in device memory, the outputs sized by a size query."""

    def __init__(self, verb, case):
        import torch
        self.torch = torch
        self.gorp = handle()
        self.parts, self.call, outputs, self.one_zero, self.per_line = VERBS[verb]
        if case == "b":
            self.parts = []
            outputs = [o for o in outputs if not o[0].endswith("_stats")]                    # (statistics without a value group are refused)
        self.kw = dict(min_lines=3) if (verb, case) == ("lines_by_key", "d") else {}
        arrays = BATCHES[case]
        self.n = len(arrays[2])
        self.host_in = arrays
        self.dev_in = [torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda() for a in arrays]
        rc, self.totals = self.run({}, device=False)                                         # the size query
        assert rc == N.GX_OK
        t = flat(self.totals)
        self.outputs = {name: (width * count(t, self.n), width) for name, width, count in outputs}

    def inputs(self, device):
        data, offsets, ids, caps = self.dev_in if device else self.host_in
        ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
        return ptr(data), ptr(offsets), self.n, ptr(ids), ptr(caps)

    def run(self, ptrs, device):
        kw = dict(self.kw, device_pointers=device, **{name + "_ptr": p for name, p in ptrs.items()})
        return self.call(self.gorp, self.inputs(device), self.parts, kw)

    def deliver(self, names, device):
        """the call with the named outputs; returns (totals, {name: the whole buffer as bytes})"""
        sizes = {name: sum(self.outputs[name]) for name in names}                            # the written part and one element
        if device:
            bufs = {name: self.torch.full((size,), POISON, dtype=self.torch.uint8, device="cuda") for name, size in sizes.items()}
            rc, totals = self.run({name: b.data_ptr() for name, b in bufs.items()}, True)
            self.torch.cuda.synchronize()                                                    # (the emit is left running on the stream)
            got = {name: b.cpu().numpy().tobytes() for name, b in bufs.items()}
        else:
            bufs = {name: np.full(size, POISON, np.uint8) for name, size in sizes.items()}
            rc, totals = self.run({name: b.ctypes.data for name, b in bufs.items()}, False)
            got = {name: b.tobytes() for name, b in bufs.items()}
        assert rc == N.GX_OK
        return totals, got

    def written(self, got, name, dtype):
        return np.frombuffer(got[name][:self.outputs[name][0]], dtype).tolist()


@pytest.mark.parametrize("case", sorted(BATCHES))
@pytest.mark.parametrize("verb", sorted(VERBS))
def test_host_arrays_and_device_pointers_hold_the_same_bytes(verb, case):
    r = Runner(verb, case)
    host_totals, host = r.deliver(list(r.outputs), device=False)
    dev_totals, dev = r.deliver(list(r.outputs), device=True)
    assert host_totals == dev_totals == r.totals
    for name, (size, width) in r.outputs.items():
        assert host[name] == dev[name], name
        assert host[name][size:] == bytes([POISON]) * width, name                            # nothing beyond the written part
    t = flat(r.totals)
    found = t[FOUND[verb]]
    if case in "abc" or (case == "d" and verb in ("lines_by_key", "group_pairs", "group_series", "bucket_lines")):
        assert found == 0
        mine = lambda names: [name for name in names if case in "abc" or not name.startswith(("key_offsets", "line_key"))]
        for name in mine(r.one_zero):
            width = r.outputs[name][1]
            entries = r.written(host, name, np.uint32 if width == 4 else np.uint64)
            assert entries == [0] * len(entries) and len(entries) == (t["n_keys"] + 1 if name.startswith("key_") else 1), name
        for name in mine(r.per_line):
            assert r.written(host, name, np.uint32) == [NONE] * r.n, name
    if case in "abc":
        assert t.get("n_keys", 0) == 0 and t.get("keyed", 0) == 0 and t["lines"] == (3 if case == "c" else 0)
    if case in "de" and "line_key" in r.outputs:
        assert t["n_keys"] == 2 and r.written(host, "line_key", np.uint32) == [0, 1, 0] and r.written(host, "key_offsets", np.uint32) == [0, 1, 2]
    if case == "e":
        assert found == {"lines_by_key": 3}.get(verb, 2)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("verb", sorted(VERBS))
def test_an_output_requested_alone_holds_what_it_holds_among_all(verb, device):
    r = Runner(verb, "e")
    totals, together = r.deliver(list(r.outputs), device)
    for name in r.outputs:
        alone_totals, alone = r.deliver([name], device)
        assert alone_totals == totals and alone[name] == together[name], name
