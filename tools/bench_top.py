#!/usr/bin/env python3
"""Developer tool: time gx_top_lines on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) ranked by
GetRequest.timeTakenInMsec for n_wanted = 10, 100 and GX_TOP_MAX_LINES -- the call with every output on the device, and its size query
-- next to gx_capture_stats of the same group on the same batch, in the same process on the same device: that pass reads the same ids,
rows, offsets and value bytes with the same parse.  The calls are timed in alternation, round by round, and the stats pass twice: the
difference between its two series is the spread a difference has to exceed.
Also printed: what the ranking is expected to add to the stats pass -- eight sweeps of the 8-byte key column and the candidate flags, and
one flags / scan / compact round -- at the device's own plain-read rate (a torch int64 sum over the line buffer, bench.py's
roofline.this_box), and measured over expected.
Times by events around repeated calls; every call synchronises once, which is part of what a caller pays.
Usage: bench_top.py [lines] [line_bytes]"""
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


def box_read_rate():
    """bench.py's box_read_rate on the line buffer, GB/s"""
    v = data[: data.numel() & ~15].view(torch.int64)
    for _ in range(3):
        v.sum()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        v.sum()
    e1.record()
    torch.cuda.synchronize()
    return v.numel() * 8 / (e0.elapsed_time(e1) / 10 * 1e-3) / 1e9


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
print("device: %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), n, lb, width))

by = g.top_parts([("GetRequest", "timeTakenInMsec")])
measures = g.measures([("GetRequest", "timeTakenInMsec")])
batch = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)
MAXN = N.GX_TOP_MAX_LINES
wanted = [w for w in (10, 100, MAXN)]
out = {w: (torch.zeros(w, dtype=torch.int32, device="cuda"), torch.zeros(w, dtype=torch.int64, device="cuda"), torch.zeros(w * lb, dtype=torch.uint8, device="cuda"),
           torch.zeros(w + 1, dtype=torch.int32, device="cuda"), torch.zeros((w, width), dtype=torch.uint8, device="cuda")) for w in wanted}


def full(w):
    o = out[w]
    return g.top_lines_device(*batch, by, w, out_index_ptr=o[0].data_ptr(), out_values_ptr=o[1].data_ptr(), out_data_ptr=o[2].data_ptr(),
                              out_offsets_ptr=o[3].data_ptr(), out_ids_ptr=o[4].data_ptr(), cap_lines=w, out_bytes_cap=w * lb, compact=2, stream=st)


def stats():
    return g.capture_stats_device(*batch, measures, compact=2, stream=st)[0]


# the calls agree with each other and with a sort of the parsed column (workloads.readme3_lines: one to four digits, so every value parses)
s = stats()
GET = names.index("GetRequest")
of_get = rows[:, 0].view(torch.int8) == GET
lines = torch.nonzero(of_get)[:, 0]
b, e = rows[of_get, 1 + 2 * 2].long(), rows[of_get, 2 + 2 * 2].long()
j = torch.arange(4, device="cuda")[None, :]
digit = data.view(n, lb)[of_get].gather(1, (b[:, None] + j).clamp(max=lb - 1)).long() - 48
v = (digit * torch.tensor([1, 10, 100, 1000], device="cuda")[((e - b)[:, None] - 1 - j).clamp(min=0)] * (j < (e - b)[:, None])).sum(1)
order = torch.sort(v, stable=True, descending=True)[1]
for w in wanted:
    rc, totals = full(w)
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["numbers"] == s["numbers"] == int(of_get.sum()) and totals["n_top"] == w
    assert torch.equal(out[w][0].long(), lines[order[:w]]) and torch.equal(out[w][1], v[order[:w]]) and int(out[w][1][0]) == s["max"]
value_units = int((e - b).sum())
stats_bytes = n * (width + 8) + value_units
cands = int(of_get.sum())
# the ranking's own traffic: the key column written for the candidates and the flag per line; eight sweeps that read the flag of every
# line and the key of a candidate; flags (read both, write 8 B per line), scan (read 8 B twice, write 8 B), compact (read 16 B per line)
sweeps = 8 * (n + 8 * cands)
extra = (8 * cands + n) + sweeps + (n + 8 * cands + 8 * n) + 24 * n + 16 * n
issue_estimate = 8 * 8 * n          # "eight sweeps of an 8-byte column" alone

rate = box_read_rate()
calls = [stats] + [lambda w=w: full(w) for w in wanted] + [lambda w=w: g.top_lines_device(*batch, by, w, compact=2, stream=st) for w in wanted] + [stats]
res = timed(calls)
ms_stats, ms_stats2 = res[0][0], res[-1][0]
spread = abs(ms_stats - ms_stats2)
print("rank by GetRequest.timeTakenInMsec: %d candidates of %d lines; plain read of the line buffer %.0f GB/s" % (cands, n, rate))
print("    gx_capture_stats (same group)      %8.3f ms (min %.3f); again %.3f ms (min %.3f): spread %.3f ms; the pass reads %.3f GB" %
      (res[0][0], res[0][1], res[-1][0], res[-1][1], spread, stats_bytes / 1e9))
base = min(ms_stats, ms_stats2)
exp_ms, exp_issue = extra / rate / 1e6, issue_estimate / rate / 1e6
print("    expected extra over the stats pass: %.3f GB = %.3f ms at the plain-read rate (eight sweeps of an 8-byte column alone: %.3f GB = %.3f ms)" %
      (extra / 1e9, exp_ms, issue_estimate / 1e9, exp_issue))
for i, w in enumerate(wanted):
    (ms, mn), (q, qn) = res[1 + i], res[1 + len(wanted) + i]
    print("    gx_top_lines n_wanted %-5d          %8.3f ms (min %.3f); size query %.3f ms (min %.3f); extra over stats %.3f ms = %.2f x expected (%.2f x the sweeps alone)" %
          (w, ms, mn, q, qn, ms - base, (ms - base) / exp_ms, (ms - base) / exp_issue))
