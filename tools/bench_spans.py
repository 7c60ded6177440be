#!/usr/bin/env python3
"""Developer tool: time gx_group_spans on N fabricated request lines on the device -- a line is its key in 6 digits, its time in 10
digits and a byte of filler, over a handle of two trivial extractions (extraction 0 begins, extraction 1 ends) with dense int32 capture
rows made here (the tests' scheme) -- with about N / 100 keys in no order at all and the roles drawn at random, so that every state
occurs.  In the same process, taking turns round by round:
  the call, every span output and line_key written to device buffers; its size query; the call under GX_BY_KEY_ALL_DIGITS;
  gx_group_sessions on the same batch with every output (the neighbouring call: one sort more, no duration columns), and gx_group_lines'
      size query (the build both stand on);
  what it replaces, from calls the library had before: gx_group_lines with device_pointers writing line_key, the download of line_key,
      numpy's stable argsort by key number and shifted compares on the host.
No ratio is fixed in advance.  Times by events around repeated calls after a warm-up, median and minimum over the rounds; every call
synchronises as often as it does for any caller, which is part of what a caller pays.
Usage: bench_spans.py [lines] [--out FILE]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd.gorp import FlattenedExtraction, Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_spans.txt")
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
pieces = [["text", "a"]] + [["extractor", "v%d" % q, [["pattern", ".*"]]] for q in range(3)]
g = Gorp.construct([FlattenedExtraction("r%d" % k, pieces) for k in range(2)])
gen = torch.Generator(device="cuda").manual_seed(2)
key = torch.randint(0, n_keys, (n,), generator=gen, device="cuda", dtype=torch.int64)
t = torch.randint(0, SPAN, (n,), generator=gen, device="cuda", dtype=torch.int64)
ids = torch.randint(0, 2, (n,), generator=gen, device="cuda", dtype=torch.int32)
data = torch.full((n, W), 0x2E, dtype=torch.uint8, device="cuda")
q = key.clone()
for d in range(KD - 1, -1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
q = t.clone()
for d in range(KD + TD - 1, KD - 1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * W).to(torch.int32)
caps = torch.tensor([0, KD, KD, KD + TD, -1, -1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
st = torch.cuda.current_stream().cuda_stream
torch.cuda.synchronize()
say("device: %s; library %s; %d lines x %d bytes, dense int32 rows; %d keys, begins and ends drawn at random"
    % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, W, n_keys))
batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
parts = g.span_parts([(0, 0, 1, "begin"), (1, 0, 1, "end")])
timed_parts = g.series_parts([(0, 0, 1), (1, 0, 1)])
i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
u8 = lambda count: torch.empty(count, dtype=torch.uint8, device="cuda")
mk, ms = 2 * n_keys, n // 2
lkey, klines = i32(n), i64(mk)
out = {"span_key": i32(ms), "span_begin_line": i32(ms), "span_end_line": i32(ms), "span_begin": i64(ms), "span_end": i64(ms), "span_duration": i64(ms),
       "span_class": u8(ms), "key_span_begin": i64(mk + 1), "key_span_stats": i64(8 * mk), "key_open_line": i32(mk), "line_span": i32(n), "line_state": u8(n)}
key_outs = dict(key_lines_ptr=klines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=mk)
ptrs = {name + "_ptr": a.data_ptr() for name, a in out.items()}


def spans(**kw):
    return g.group_spans_device(*batch, parts, max_spans=ms, stream=st, **key_outs, **ptrs, **kw)


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


rc, totals = spans()
torch.cuda.synchronize()
assert rc == N.GX_OK and totals["exact"] and totals["keyed"] == totals["lines"] == n, (rc, totals)
ns = totals["n_spans"]
say("%d keys, %d spans (%.2f per key), %d begins superseded, %d left open, %d ends without a begin"
    % (totals["n_keys"], ns, ns / totals["n_keys"], totals["superseded"], totals["left_open"], totals["orphan_ends"]))


def host_path():
    """what a caller did before: group_lines for line_key, the download, a stable argsort by key number, shifted compares"""
    rc, _ = g.group_lines_device(*batch, parts[0], stream=st, **key_outs)
    k, role = lkey.cpu().numpy().view(np.uint32), ids.cpu().numpy()
    order = np.argsort(k, kind="stable")
    ks, rs = k[order], role[order]
    end = np.concatenate([[False], (ks[1:] == ks[:-1]) & (rs[1:] == 1) & (rs[:-1] == 0)])
    return order, end


order, end = host_path()
assert int(end.sum()) == ns and np.array_equal(order[end].astype(np.uint32), out["span_end_line"][:ns].cpu().numpy().view(np.uint32))
t0 = time.perf_counter(); host_path(); t_host = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter(); lkey.cpu(); ids.cpu(); torch.cuda.synchronize(); t_down = (time.perf_counter() - t0) * 1e3

sess = {"session_key": i32(n), "session_begin": i64(n), "session_end": i64(n), "session_first_line": i32(n), "session_lines": i64(n),
        "session_entry_begin": i64(n + 1), "key_session_begin": i64(mk + 1), "entry_line": i32(n), "line_session": i32(n)}
sess_ptrs = {name + "_ptr": a.data_ptr() for name, a in sess.items()}
sessions = lambda: g.group_sessions_device(*batch, timed_parts, SPAN * 35 // 1000, max_sessions=n, max_entries=n, stream=st, **key_outs, **sess_ptrs)
rc, stotals = sessions()
torch.cuda.synchronize()
assert rc == N.GX_OK and stotals["entries"] == n, (rc, stotals)
calls = [spans, lambda: g.group_spans_device(*batch, parts, max_keys=mk, stream=st), lambda: spans(all_digits=True), sessions,
         lambda: g.group_lines_device(*batch, parts[0], max_keys=mk, stream=st)]
res = timed(calls)
labels = ["gx_group_spans, every output", "gx_group_spans, size query", "gx_group_spans, every output, all digits",
          "gx_group_sessions, every output, %d sessions" % stotals["n_sessions"], "gx_group_lines, size query"]
for label, (med, mn) in zip(labels, res):
    say("    %-48s %9.3f ms (min %.3f)" % (label, med, mn))
say("    the parts of the call, by difference of medians: the build it stands on %.3f ms; entries pass, sort, heads, scans %.3f ms; emits %.3f ms"
    % (res[4][0], res[1][0] - res[4][0], res[0][0] - res[1][0]))
say("    gx_group_spans / gx_group_sessions = %.2f" % (res[0][0] / res[3][0]))
say("    replaced: gx_group_lines + download of line_key and the ids + numpy stable argsort + compares   %9.1f ms (of it the two downloads %.1f ms)" % (t_host, t_down))
say("    host path / gx_group_spans = %.0f" % (t_host / res[0][0]))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
