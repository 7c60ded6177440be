#!/usr/bin/env python3
"""Developer tool: time gx_group_series on config 2 (README definition, N x 200-byte lines on the device, u8 result rows), the lines'
nine-digit timestamps rewritten in place (the result rows hold offsets alone and stay valid), keyed by `verb` (6 keys) and bucketed by
`timestamp`, in two shapes
  (a) time-ordered, timestamp = line number, about 20 buckets: verb x 20 minutes, about 120 cells -- the dashboard panel;
  (b) time-ordered, about 15 000 buckets: about 90 000 cells;
each next to, in the same process and alternating round by round, the two calls a caller had to make before (and which still did not
answer the question): gx_group_lines by verb and gx_bucket_lines by timestamp on the same batch -- the yardsticks, code this call does not
touch.  The expectation for (a), stated before anything was measured: the call reads the batch twice, as those two calls do together --
once in the unchanged k_group_build and once in a build that does k_bucket_build's work on the lines that have a key -- so with every
output its median should be no more than the SUM of the two yardsticks' medians plus that run's own min-to-median spread of that sum.
(b) carries no bound.  Every shape is timed as the full call (every key output and every series output written to device buffers) and as
the size query.  Times by events around repeated calls after a warm-up, median and minimum over the rounds; every call synchronises once,
which is part of what a caller pays.
Usage: bench_group_series.py [lines] [line_bytes] [--out FILE] [--append] [--cases ab]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_series.txt")
append, cases = False, "ab"
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--append" in argv:
    argv.remove("--append"); append = True
if "--cases" in argv:
    at = argv.index("--cases"); cases = argv[at + 1]; del argv[at:at + 2]
n = int(argv[0]) if len(argv) > 0 else 10_000_000
lb = int(argv[1]) if len(argv) > 1 else W.LINE_BYTES
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


g = Gorp.construct(W.readme3_definition())
names = [x.getName() for x in g.getExtractions()]
data, off, cat = W.readme3_lines(n, seed=2, device="cuda", line_bytes=lb)
width = 1 + 2 * g.max_groups
rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb, max_line_bytes=lb, compact=2)
torch.cuda.synchronize()
assert torch.equal(rows[:, 0].view(torch.int8).to(torch.int32), cat.to(torch.int32))
say("device: %s; library %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, lb, width))
batch = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)
matched = int((cat >= 0).sum())
assert n <= 10 ** 9
verb_parts = g.group_parts([(name, "verb") for name in names])
ts_parts = g.bucket_parts([(name, "timestamp") for name in names])
series_parts = g.series_parts([(name, "verb", "timestamp") for name in names])


def stamp(ts):
    """the lines' timestamps: ts[i] in nine digits, zero-padded, in place"""
    view = data.view(n, lb)
    q = ts.clone()
    for d in range(9, 0, -1):
        view[:, d] = (48 + q % 10).to(torch.uint8)
        q //= 10
    torch.cuda.synchronize()


def timed(calls, reps=5, rounds=7):
    """median and minimum ms per call of every call in `calls`, the calls taking turns round by round"""
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need 25 ms of unbroken load: profiles/r04_clock_ramp.txt)
    while time.perf_counter() < t_spin:
        for call in calls:
            call()
        torch.cuda.synchronize()
    ts = [[] for _ in calls]
    for _ in range(rounds):
        for c, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record(); torch.cuda.synchronize()
            ts[c].append(e0.elapsed_time(e1) / reps)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def case(label, what, bucket_width, max_cells, bound):
    i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
    i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
    units, koff, kfirst, klines, lkey = torch.empty(1024, dtype=torch.uint8, device="cuda"), i32(65), i32(64), i64(64), i32(n)
    number, ckey, cbucket, cfirst, clines, begin, lcell = i64(max_cells), i32(max_cells), i32(max_cells), i32(max_cells), i64(max_cells), i64(65), i32(n)
    bnumber, bfirst, blines, lbucket = i64(max_cells), i32(max_cells), i64(max_cells), i32(n)
    key_outs = dict(key_units_ptr=units.data_ptr(), key_units_cap=1024, key_offsets_ptr=koff.data_ptr(), key_first_line_ptr=kfirst.data_ptr(),
                    key_lines_ptr=klines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=64)
    full = lambda: g.group_series_device(*batch, series_parts, bucket_width, bucket_number_ptr=number.data_ptr(), cell_key_ptr=ckey.data_ptr(),
                                         cell_bucket_ptr=cbucket.data_ptr(), cell_first_line_ptr=cfirst.data_ptr(), cell_lines_ptr=clines.data_ptr(),
                                         key_cell_begin_ptr=begin.data_ptr(), line_cell_ptr=lcell.data_ptr(), max_cells=max_cells, max_buckets=max_cells, compact=2,
                                         stream=st, **key_outs)
    query = lambda: g.group_series_device(*batch, series_parts, bucket_width, max_keys=64, max_cells=max_cells, compact=2, stream=st)
    yard_g = lambda: g.group_lines_device(*batch, verb_parts, compact=2, stream=st, **key_outs)
    yard_b = lambda: g.bucket_lines_device(*batch, ts_parts, bucket_width, bucket_number_ptr=bnumber.data_ptr(), bucket_first_line_ptr=bfirst.data_ptr(),
                                           bucket_lines_ptr=blines.data_ptr(), line_bucket_ptr=lbucket.data_ptr(), max_buckets=max_cells, compact=2, stream=st)
    rc, totals = full()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["exact"] and totals["cells_exact"] and totals["lines"] == totals["celled"] == matched and totals["n_keys"] == 6, (rc, totals)
    c, b = totals["n_cells"], totals["n_buckets"]
    word = ckey[:c].to(torch.int64) * b + cbucket[:c]
    assert int(clines[:c].sum()) == matched and bool((torch.diff(word) > 0).all()) and bool((torch.diff(number[:b]) > 0).all()) and int(begin[6]) == c
    assert bool(((lcell == -1) == (cat < 0)).all())
    rc, alone = yard_b()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and alone["n_buckets"] == b and bool((bnumber[:b] == number[:b]).all())
    (ms_full, mn_full), (ms_query, mn_query), (ms_g, mn_g), (ms_b, mn_b) = timed([full, query, yard_g, yard_b])
    say("(%s) %s, width %d: %d cells = 6 verbs x %d buckets (%d .. %d) over %d lines" % (label, what, bucket_width, c, b, totals["first_bucket"], totals["last_bucket"], matched))
    say("    gx_group_series, every output            %8.3f ms (min %.3f)" % (ms_full, mn_full))
    say("    gx_group_series, size query              %8.3f ms (min %.3f)" % (ms_query, mn_query))
    say("    gx_group_lines by verb, every output     %8.3f ms (min %.3f)" % (ms_g, mn_g))
    say("    gx_bucket_lines by timestamp, every out  %8.3f ms (min %.3f)" % (ms_b, mn_b))
    total, spread = ms_g + ms_b, (ms_g + ms_b) - (mn_g + mn_b)
    say("    group_series / (group_lines + bucket_lines) = %.2f%s"
        % (ms_full / total, "; the expectation: no more than the sum of the two medians plus its min-to-median spread, %.3f + %.3f ms -- %s"
           % (total, spread, "MET" if ms_full <= total + spread else "MISSED") if bound else "; no bound"))


stamp(torch.arange(n, dtype=torch.int64, device="cuda"))
if "a" in cases:
    case("a", "time-ordered", max(1, n // 20), 1024, True)
if "b" in cases:
    case("b", "time-ordered", max(1, n // 15000), 1 << 17, False)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(report) + "\n")
