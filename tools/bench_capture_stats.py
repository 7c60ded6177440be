#!/usr/bin/env python3
"""Developer tool: time gx_capture_stats on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) with one
measure, GetRequest.timeTakenInMsec with 16 histogram edges, next to two yardsticks in the same process on the same device:
  - the size query of gx_select_lines_where with the single term GetRequest.timeTakenInMsec >= 0: the same ids, rows, offsets and
    value bytes read and the same parse, then 5 B/line of flags written and two scans that the stats call does not have;
  - gx_count_outcomes: a read of the id column alone.
Also printed: the algorithmic bytes of the stats pass -- id and row, two offsets per line, and the code units of the measured values.
Times by events around repeated calls; every call synchronises once, which is part of what a caller pays.
Usage: bench_capture_stats.py [lines] [line_bytes]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
lb = int(sys.argv[2]) if len(sys.argv) > 2 else W.LINE_BYTES
g = Gorp.construct(W.readme3_definition())
names = [x.getName() for x in g.getExtractions()]
data, off, cat = W.readme3_lines(n, seed=2, device="cuda", line_bytes=lb)
width = 1 + 2 * g.max_groups
rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream


def timed(call, reps=10, rounds=7):
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need 25 ms of unbroken load: profiles/r04_clock_ramp.txt)
    while time.perf_counter() < t_spin:
        call()
        torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return sorted(ts)[len(ts) // 2], min(ts)


g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb, max_line_bytes=lb, compact=2)
torch.cuda.synchronize()
assert torch.equal(rows[:, 0].view(torch.int8).to(torch.int32), cat.to(torch.int32))
print("device: %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), n, lb, width))

EDGES = [1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 3000, 4000, 5000, 7500, 9000]
measures = g.measures([("GetRequest", "timeTakenInMsec", EDGES)])
terms = g.where_terms([("GetRequest", "timeTakenInMsec", ">=", 0)])
mask = g._where_want(terms, "matched-by-terms")
batch = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)

stats = g.capture_stats_device(*batch, measures, compact=2, stream=st)[0]
k, nbytes = g.select_lines_where_device(*batch, mask, terms, compact=2, stream=st)
counts = g.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=st)
GET = names.index("GetRequest")
# the three calls agree with each other and with the generator (workloads.readme3_lines: one to four digits, so every value parses)
assert stats["lines"] == stats["numbers"] == k == int(counts[GET]) == int((cat == GET).sum()) and int(stats["hist"].sum()) == k
of_get = rows[:, 0].view(torch.int8) == GET
b, e = rows[of_get, 1 + 2 * 2].long(), rows[of_get, 2 + 2 * 2].long()
value_units = int((e - b).sum())
pass_bytes = n * (width + 8) + value_units

ms_stats, mn_stats = timed(lambda: g.capture_stats_device(*batch, measures, compact=2, stream=st))
ms_where, mn_where = timed(lambda: g.select_lines_where_device(*batch, mask, terms, compact=2, stream=st))
ms_count, mn_count = timed(lambda: g.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=st))
print("measure GetRequest.timeTakenInMsec, %d edges: %d lines, %d numbers, min %d, max %d, sum %d" % (len(EDGES), stats["lines"], stats["numbers"], stats["min"],
                                                                                                      stats["max"], stats["sum"]))
print("    hist %s" % stats["hist"].tolist())
print("    gx_capture_stats                   %8.3f ms (min %.3f); the pass reads %.3f GB (%.3f GB of values): %.0f GB/s" %
      (ms_stats, mn_stats, pass_bytes / 1e9, value_units / 1e9, pass_bytes / 1e6 / ms_stats))
print("    gx_select_lines_where size query   %8.3f ms (min %.3f); term GetRequest.timeTakenInMsec >= 0, %d lines kept" % (ms_where, mn_where, k))
print("    gx_count_outcomes                  %8.3f ms (min %.3f)" % (ms_count, mn_count))
print("    capture_stats / size query = %.3f (the bound: 1.25); capture_stats - count_outcomes = %.3f ms" % (ms_stats / ms_where, ms_stats - ms_count))
