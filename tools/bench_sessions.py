#!/usr/bin/env python3
"""Developer tool: time gx_group_sessions on N fabricated request lines on the device -- a line is its key in 6 digits, its time in 10
digits and a byte of filler, over a handle of one trivial extraction with dense int32 capture rows made here (the tests' scheme) -- with
about N / 100 keys in no order at all and a gap that yields a few sessions per key.  In the same process, taking turns round by round:
  the call, every session output and line_key written to device buffers; its size query; both under GX_BUCKET_ALL_DIGITS (the second arm
      of the digit plan);
  the call's parts, by events around calls that stop earlier: gx_group_lines' size query on the same batch (the build it stands on),
      the sessions' size query (+ the keys pass, both sorts, the heads, their scan, the longest), the full call (+ the emits);
  what it replaces, from calls the library had before: gx_group_lines with device_pointers writing line_key, the download of line_key and
      of the times' column, numpy lexsort + diff on the host;
  gx_group_series on the same batch (fixed intervals of the gap's width), a yardstick of the passes the two calls share.
No ratio is fixed in advance.  Times by events around repeated calls after a warm-up, median and minimum over the rounds; every call
synchronises as often as it does for any caller, which is part of what a caller pays.
Usage: bench_sessions.py [lines] [--out FILE]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd.gorp import FlattenedExtraction, Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_sessions.txt")
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
n = int(argv[0]) if argv else 10_000_000
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


KD, TD = 6, 10
W = KD + TD + 1
n_keys = max(1, n // 100)
SPAN = 10 ** 9
GAP = SPAN * 35 // 1000        # 100 entries per key over SPAN: about 1 + 100 exp(-3.5) = 4 sessions per key
g = Gorp.construct([FlattenedExtraction("r0", [["text", "a"]] + [["extractor", "v%d" % q, [["pattern", ".*"]]] for q in range(3)])])
gen = torch.Generator(device="cuda").manual_seed(2)
key = torch.randint(0, n_keys, (n,), generator=gen, device="cuda", dtype=torch.int64)
t = torch.randint(0, SPAN, (n,), generator=gen, device="cuda", dtype=torch.int64)
data = torch.full((n, W), 0x2E, dtype=torch.uint8, device="cuda")
q = key.clone()
for d in range(KD - 1, -1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
q = t.clone()
for d in range(KD + TD - 1, KD - 1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * W).to(torch.int32)
ids = torch.zeros(n, dtype=torch.int32, device="cuda")
caps = torch.tensor([0, KD, KD, KD + TD, -1, -1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
st = torch.cuda.current_stream().cuda_stream
torch.cuda.synchronize()
say("device: %s; library %s; %d lines x %d bytes, dense int32 rows; %d keys, max_gap %d over a span of %d"
    % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, W, n_keys, GAP, SPAN))
batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
parts = g.series_parts([(0, 0, 1)])
i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
mk = 2 * n_keys
lkey, klines = i32(n), i64(mk)
out = {"session_key": i32(n), "session_begin": i64(n), "session_end": i64(n), "session_first_line": i32(n), "session_lines": i64(n),
       "session_entry_begin": i64(n + 1), "key_session_begin": i64(mk + 1), "entry_line": i32(n), "line_session": i32(n)}
key_outs = dict(key_lines_ptr=klines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=mk)
ptrs = {name + "_ptr": a.data_ptr() for name, a in out.items()}


def sessions(**kw):
    return g.group_sessions_device(*batch, parts, GAP, max_sessions=n, max_entries=n, stream=st, **key_outs, **ptrs, **kw)


def timed(calls, reps=3, rounds=7):
    """median and minimum ms per call of every call in `calls`, the calls taking turns round by round"""
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need unbroken load before they are up)
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
    return [(sorted(x)[len(x) // 2], min(x)) for x in ts]


rc, totals = sessions()
torch.cuda.synchronize()
assert rc == N.GX_OK and totals["exact"] and totals["entries"] == totals["lines"] == n, (rc, totals)
ns = totals["n_sessions"]
say("%d keys, %d sessions (%.2f per key), the longest %d entries" % (totals["n_keys"], ns, ns / totals["n_keys"], totals["longest_lines"]))


def host_path():
    """what a caller did before: group_lines for line_key, both columns to the host, lexsort, diff"""
    rc, _ = g.group_lines_device(*batch, parts[0], stream=st, **key_outs)
    k, tt = lkey.cpu().numpy().view(np.uint32), t.cpu().numpy()
    order = np.lexsort((tt, k))          # (stable: ties by line)
    ks, tts = k[order], tt[order]
    head = np.concatenate([[True], (np.diff(ks) != 0) | (np.diff(tts.astype(np.uint64)) > np.uint64(GAP))])
    return order, head


order, head = host_path()
assert int(head.sum()) == ns and np.array_equal(order.astype(np.uint32), out["entry_line"][:n].cpu().numpy().view(np.uint32))
t0 = time.perf_counter(); host_path(); t_host = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter(); lkey.cpu(); t.cpu(); torch.cuda.synchronize(); t_down = (time.perf_counter() - t0) * 1e3

calls = [sessions, lambda: g.group_sessions_device(*batch, parts, GAP, max_keys=mk, stream=st),
         lambda: sessions(all_digits=True), lambda: g.group_sessions_device(*batch, parts, GAP, max_keys=mk, stream=st, all_digits=True),
         lambda: g.group_lines_device(*batch, parts[0], max_keys=mk, stream=st), lambda: g.group_lines_device(*batch, parts[0], stream=st, **key_outs)]
cells = 1 << 22
series_out = dict(cell_key_ptr=i32(cells).data_ptr(), cell_bucket_ptr=i32(cells).data_ptr(), cell_lines_ptr=i64(cells).data_ptr(), line_cell_ptr=i32(n).data_ptr(),
                  key_cell_begin_ptr=i64(mk + 1).data_ptr(), bucket_number_ptr=i64(cells).data_ptr())
series = lambda: g.group_series_device(*batch, parts, GAP, max_cells=cells, max_buckets=cells, stream=st, **key_outs, **series_out)
rc, stotals = series()
torch.cuda.synchronize()
if rc == N.GX_OK:
    calls.append(series)
res = timed(calls)
labels = ["gx_group_sessions, every output", "gx_group_sessions, size query", "... every output, all digits", "... size query, all digits",
          "gx_group_lines, size query", "gx_group_lines, line_key + key_lines", "gx_group_series, width = max_gap, %d cells" % stotals["n_cells"]]
for label, (med, mn) in zip(labels, res):
    say("    %-48s %9.3f ms (min %.3f)" % (label, med, mn))
say("    the parts of the call, by difference of medians: the build it stands on %.3f ms; keys pass, sorts, heads, scan, longest %.3f ms; emits %.3f ms"
    % (res[4][0], res[1][0] - res[4][0], res[0][0] - res[1][0]))
say("    replaced: gx_group_lines + download of line_key and the times + numpy lexsort + diff     %9.1f ms (of it the two downloads %.1f ms)" % (t_host, t_down))
say("    host path / gx_group_sessions = %.0f" % (t_host / res[0][0]))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
