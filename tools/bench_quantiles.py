#!/usr/bin/env python3
"""Developer tool: time gx_capture_quantiles on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) by
GetRequest.timeTakenInMsec with 1, 3 (50/100, 95/100, 99/100) and 16 quantiles, next to its neighbours on the same batch, in the same
process on the same device: gx_capture_stats of the same group, and gx_top_lines with n_wanted = 10 as a size query -- the yardstick:
the same keys pass, and an eight-digit select over the per-line columns with three launches a digit.  The calls are timed in
alternation, round by round, and the yardstick twice, before and behind the quantile calls: the difference between its two series is the
spread a difference has to exceed.
Times by events around repeated calls; every call synchronises once, which is part of what a caller pays.
GX_BENCH_LIB=<path> times another build of the library (build.py --variant nocompact -DGX_QUANT_NO_COMPACT: the other arm).
Usage: bench_quantiles.py [lines] [line_bytes]"""
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


def timed(calls, reps=10, rounds=7):
    """median and minimum ms per call of every call, the calls taking turns round by round"""
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need 25 ms of unbroken load: profiles/r04_clock_ramp.txt)
    while time.perf_counter() < t_spin:
        for call in calls:                # (and every shape of the timed window is warmed up)
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


g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb, max_line_bytes=lb, compact=2)
torch.cuda.synchronize()
assert torch.equal(rows[:, 0].view(torch.int8).to(torch.int32), cat.to(torch.int32))
print("device: %s; %d lines x %d bytes, u8 result rows of %d bytes; library %s" % (torch.cuda.get_device_name(0), n, lb, width, os.path.basename(N.LIB_PATH)))

by = g.top_parts([("GetRequest", "timeTakenInMsec")])
measures = g.measures([("GetRequest", "timeTakenInMsec")])
batch = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)
asks = {1: [(50, 100)], 3: [(50, 100), (95, 100), (99, 100)], 16: [(j + 1, 17) for j in range(16)]}


def stats():
    return g.capture_stats_device(*batch, measures, compact=2, stream=st)[0]


def top10():
    return g.top_lines_device(*batch, by, 10, compact=2, stream=st)


def quantiles(k):
    return g.capture_quantiles_device(*batch, by, asks[k], compact=2, stream=st)


# the calls agree with each other and with a sort of the parsed column (workloads.readme3_lines: one to four digits, so every value parses)
s = stats()
GET = names.index("GetRequest")
of_get = rows[:, 0].view(torch.int8) == GET
b, e = rows[of_get, 1 + 2 * 2].long(), rows[of_get, 2 + 2 * 2].long()
j = torch.arange(4, device="cuda")[None, :]
digit = data.view(n, lb)[of_get].gather(1, (b[:, None] + j).clamp(max=lb - 1)).long() - 48
v = (digit * torch.tensor([1, 10, 100, 1000], device="cuda")[((e - b)[:, None] - 1 - j).clamp(min=0)] * (j < (e - b)[:, None])).sum(1)
ordered = torch.sort(v)[0]
cands = int(of_get.sum())
for k in asks:
    results, totals = quantiles(k)
    assert totals["numbers"] == s["numbers"] == cands
    for (num, den), r in zip(asks[k], results):
        rank = max(1, -(-num * cands // den))
        value = int(ordered[rank - 1])
        assert r == {"value": value, "rank": rank, "below": int((v < value).sum()), "equal": int((v == value).sum())}, (num, den, r)
ends = g.capture_quantiles_device(*batch, by, [(0, 1), (1, 1)], compact=2, stream=st)[0]
assert ends[0]["value"] == s["min"] and ends[1]["value"] == s["max"]

calls = [stats, top10] + [lambda k=k: quantiles(k) for k in asks] + [top10, stats]
res = timed(calls)
yard, yard2 = res[1][0], res[-2][0]
spread = abs(yard - yard2)
print("by GetRequest.timeTakenInMsec: %d numbers of %d lines" % (cands, n))
print("    gx_capture_stats (same group)            %8.3f ms (min %.3f); again %.3f ms (min %.3f)" % (res[0][0], res[0][1], res[-1][0], res[-1][1]))
print("    gx_top_lines n_wanted 10, size query     %8.3f ms (min %.3f); again %.3f ms (min %.3f): spread %.3f ms" % (yard, res[1][1], yard2, res[-2][1], spread))
for i, k in enumerate(asks):
    ms, mn = res[2 + i]
    print("    gx_capture_quantiles, %2d quantile%s      %8.3f ms (min %.3f); %+.3f ms against the faster yardstick series" %
          (k, " " if k == 1 else "s", ms, mn, ms - min(yard, yard2)))
ms3 = res[3][0]
bound = min(yard, yard2) + spread   # (the yardstick, and no margin but the spread between its own two series)
print("    the condition (3 quantiles <= the yardstick + its spread): %s (%.3f against %.3f)" % ("holds" if ms3 <= bound else "DOES NOT HOLD", ms3, bound))
