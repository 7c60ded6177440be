#!/usr/bin/env python3
"""Developer tool: what a number format other than LONG costs the passes that parse a captured value (gx_set_number_format).  The
syslog workload (workloads.syslog_definition, 200-byte lines; a host sample tiled on the device to N lines, dense int32 rows), and in
the same run on the same lines:
  - gx_capture_stats of `ts` read as ISO8601(0) in every extraction, next to gx_capture_stats of `pid`, a LONG group: the same ids, rows
    and offsets read, a 20-unit stamp parsed where the other call parses a number of 1 .. 5 digits;
  - gx_select_lines_where's size query with ts >= "2026-01-05T05:00:00Z", next to pid >= 32768: each keeps about half of the lines.
Reported: both times and the ratio ISO8601 / LONG.  The passes stream the batch once, so the expectation to confirm or refute is a ratio
near 1.  The answers are checked against numpy on the sample first.  Times by events around repeated calls; every call synchronises
once, which is part of what a caller pays.  Usage: bench_number.py [rules] [lines]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp, parse_number

nrules = int(sys.argv[1]) if len(sys.argv) > 1 else 16
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
rules, meta = W.syslog_definition(nrules, seed=3)
g = Gorp.construct(rules)
names = [x.getName() for x in g.getExtractions()]
for name in names:
    g.set_number_format(name, "ts", "iso8601", 0)
base_n = 100_000
data, off, cats = W.syslog_lines(meta, base_n, seed=3)
reps = max(1, n // base_n)
total = int(off[-1])
assert total * reps < 2 ** 32
d = torch.from_numpy(data.copy()).cuda().repeat(reps)
o = (torch.from_numpy(off[:-1].astype(np.int64)).cuda()[None, :] + torch.arange(reps, device="cuda", dtype=torch.int64)[:, None] * total).reshape(-1)
o = torch.cat([o, torch.tensor([total * reps], device="cuda", dtype=torch.int64)]).to(torch.uint32)
n = base_n * reps
ids = torch.empty(n, dtype=torch.int32, device="cuda")
caps = torch.empty((n, 2 * g.max_groups), dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
g.extract_batch_device(d.data_ptr(), o.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), stream=st, line_bytes_hint=W.LINE_BYTES)
torch.cuda.synchronize()
print("device: %s; %d extractions, %d lines of %.0f bytes, dense rows of %d offsets" % (torch.cuda.get_device_name(0), nrules, n, total / base_n, 2 * g.max_groups))


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
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


batch = (d.data_ptr(), o.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
MID = "2026-01-05T05:00:00Z"
m_ts, m_pid = g.measures([(name, "ts") for name in names]), g.measures([(name, "pid") for name in names])
w_ts, w_pid = g.where_terms([(name, "ts", ">=", MID) for name in names]), g.where_terms([(name, "pid", ">=", 32768) for name in names])
mask = g._where_want(w_ts, "matched-by-terms")

# the answers on the first copy of the sample, against numpy and the host's rule
h_ids, h_caps = ids[:base_n].cpu().numpy(), caps[:base_n].cpu().numpy()
stamps, pids = [], []
for i in np.flatnonzero(h_ids >= 0):
    a = int(off[i])
    stamps.append(parse_number("iso8601", 0, bytes(data[a + h_caps[i, 0]:a + h_caps[i, 1]])))
    pids.append(int(bytes(data[a + h_caps[i, 4]:a + h_caps[i, 5]])))
s_ts, s_pid = g.capture_stats_device(*batch, m_ts), g.capture_stats_device(*batch, m_pid)
numbers = [v for v in stamps if v is not None]
assert sum(s["numbers"] for s in s_ts) == len(numbers) * reps and sum(s["not_numbers"] for s in s_ts) == (len(stamps) - len(numbers)) * reps
assert min(s["min"] for s in s_ts) == min(numbers) and max(s["max"] for s in s_ts) == max(numbers) and sum(s["sum"] for s in s_ts) == sum(numbers) * reps
assert sum(s["numbers"] for s in s_pid) == len(pids) * reps and sum(s["sum"] for s in s_pid) == sum(pids) * reps
k_ts, _ = g.select_lines_where_device(*batch, mask, w_ts)
k_pid, _ = g.select_lines_where_device(*batch, mask, w_pid)
since = parse_number("iso8601", 0, MID)
assert k_ts == sum(1 for v in numbers if v >= since) * reps and k_pid == sum(1 for v in pids if v >= 32768) * reps

results = {}
for label, call in (("capture_stats ts ISO8601(0)", lambda: g.capture_stats_device(*batch, m_ts)), ("capture_stats pid LONG", lambda: g.capture_stats_device(*batch, m_pid)),
                    ("select_lines_where ts >= %s" % MID, lambda: g.select_lines_where_device(*batch, mask, w_ts)),
                    ("select_lines_where pid >= 32768", lambda: g.select_lines_where_device(*batch, mask, w_pid))):
    results[label] = timed(call)
    print("    %-48s %8.3f ms (min %.3f, max %.3f)" % ((label,) + results[label]))
t = [results[label][0] for label in results]
print("    %d of %d stamps are numbers; ts >= keeps %.1f %% of the lines, pid >= %.1f %%" % (len(numbers), len(stamps), 100.0 * k_ts / n, 100.0 * k_pid / n))
print("    ISO8601 / LONG: capture_stats %.3f, select_lines_where size query %.3f" % (t[0] / t[1], t[2] / t[3]))
