#!/usr/bin/env python3
"""Developer tool: time gx_group_windows on N fabricated login lines on the device -- a line is its key in 6 digits, its time in 10 digits
and a byte of filler, over a handle of one trivial extraction with dense int32 capture rows made here (the tests' scheme) -- with about
N / 100 keys in no order at all, a window that holds a few of a key's 100 entries and a threshold that some keys reach.  In the same
process, taking turns round by round:
  the call, every window output and line_key written to device buffers; its size query; both under GX_BUCKET_ALL_DIGITS;
  the size query with a SHORT window (every window is the entry itself: the gallop's first probe fails) and with a WHOLE-RUN window
      (every window is the key's run so far: the gallop reaches the key's first entry) -- the two ends of the window pass' cost;
  the call's parts, by events around calls that stop earlier: gx_group_lines' size query on the same batch (the build it stands on), the
      windows' size query (+ the keys pass, both sorts, the window pass, flags, scan, trips), the full call (+ the emits);
  gx_group_sessions on the same batch and device, every output and its size query: the yardstick, since the two calls share the keys
      pass and both sorts;
  the host path, for scale: gx_group_lines with device_pointers writing line_key, the download of line_key and of the times' column,
      numpy lexsort, and the caller's deque loop over the first million entries of that order.
--trace short|whole|mid runs the size query alone a few times with that window, for a kernel trace taken around the tool (the window
pass' own kernel time is k_win_lo's row there).  No ratio is fixed in advance.  Times by events around repeated calls after a warm-up,
median and minimum over the rounds; every call synchronises as often as it does for any caller, which is part of what a caller pays.
Usage: bench_windows.py [lines] [--out FILE] [--trace short|whole|mid]"""
import os, sys, time
from collections import deque
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd.gorp import FlattenedExtraction, Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_windows.txt")
trace = None
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--trace" in argv:
    at = argv.index("--trace"); trace = argv[at + 1]; del argv[at:at + 2]
n = int(argv[0]) if argv else 10_000_000
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


KD, TD = 6, 10
W = KD + TD + 1
n_keys = max(1, n // 100)
SPAN = 10 ** 9
WINDOW = SPAN * 35 // 1000     # 100 entries per key over SPAN: 3.5 further entries a window on average
THRESHOLD = 8
SHORT, WHOLE = 0, SPAN
SESSIONS_GAP = WINDOW          # (tools/bench_sessions.py's)
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
batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
parts = g.series_parts([(0, 0, 1)])
mk = 2 * n_keys
query = lambda window, **kw: g.group_windows_device(*batch, parts, window, THRESHOLD, max_keys=mk, stream=st, **kw)

if trace:
    window = {"short": SHORT, "whole": WHOLE, "mid": WINDOW}[trace]
    for _ in range(5):
        rc, totals = query(window)
        assert rc == N.GX_OK
    torch.cuda.synchronize()
    print("trace %s: window %d, %d entries, peak %d, %d trips" % (trace, window, totals["entries"], totals["peak_lines"], totals["n_trips"]))
    sys.exit(0)

say("device: %s; library %s; %d lines x %d bytes, dense int32 rows; %d keys, window %d over a span of %d, threshold %d"
    % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, W, n_keys, WINDOW, SPAN, THRESHOLD))
i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
lkey, klines = i32(n), i64(mk)
out = {"entry_line": i32(n), "entry_key": i32(n), "entry_time": i64(n), "entry_window_lines": i32(n), "key_entry_begin": i64(mk + 1), "key_peak_lines": i32(mk),
       "key_peak_line": i32(mk), "line_window_lines": i32(n), "trip_key": i32(n), "trip_line": i32(n), "trip_time": i64(n), "trip_entry": i32(n),
       "key_trip_begin": i64(mk + 1)}
key_outs = dict(key_lines_ptr=klines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=mk)
ptrs = {name + "_ptr": a.data_ptr() for name, a in out.items()}


def windows(**kw):
    return g.group_windows_device(*batch, parts, WINDOW, THRESHOLD, max_entries=n, max_trips=n, stream=st, **key_outs, **ptrs, **kw)


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


rc, totals = windows()
torch.cuda.synchronize()
assert rc == N.GX_OK and totals["exact"] and totals["entries"] == totals["lines"] == n, (rc, totals)
nt = totals["n_trips"]
say("%d keys, %d trips of %d keys, the peak %d lines in a window" % (totals["n_keys"], nt, totals["tripped_keys"], totals["peak_lines"]))
_, t_short = query(SHORT)
_, t_whole = query(WHOLE)
say("short window %d: peak %d; whole-run window %d: peak %d" % (SHORT, t_short["peak_lines"], WHOLE, t_whole["peak_lines"]))


def host_path(deque_entries=1_000_000):
    """what a caller did before: group_lines for line_key, both columns to the host, lexsort, the deque loop (over the first entries)"""
    rc, _ = g.group_lines_device(*batch, parts[0], stream=st, **key_outs)
    t0 = time.perf_counter()
    k, tt = lkey.cpu().numpy().view(np.uint32), t.cpu().numpy()
    t1 = time.perf_counter()
    order = np.lexsort((tt, k))          # (stable: ties by line)
    t2 = time.perf_counter()
    m = min(deque_entries, n)
    ks, tts = k[order][:m].tolist(), tt[order][:m].tolist()
    wl = [0] * m
    qd, prev = deque(), None
    for e in range(m):
        if ks[e] != prev:
            qd.clear(); prev = ks[e]
        te = tts[e]
        qd.append(te)
        while te - qd[0] > WINDOW:
            qd.popleft()
        wl[e] = len(qd)
    t3 = time.perf_counter()
    return order, wl, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, m


order, wl, t_down, t_sort, t_deque, m_deque = host_path()
assert np.array_equal(order.astype(np.uint32), out["entry_line"][:n].cpu().numpy().view(np.uint32))
assert wl == out["entry_window_lines"][:m_deque].cpu().numpy().view(np.uint32).tolist()

sess = {"session_key": i32(n), "session_begin": i64(n), "session_end": i64(n), "session_first_line": i32(n), "session_lines": i64(n),
        "session_entry_begin": i64(n + 1), "key_session_begin": i64(mk + 1), "entry_line": i32(n), "line_session": i32(n)}
sptrs = {name + "_ptr": a.data_ptr() for name, a in sess.items()}
calls = [windows, lambda: query(WINDOW), lambda: windows(all_digits=True), lambda: query(WINDOW, all_digits=True), lambda: query(SHORT), lambda: query(WHOLE),
         lambda: g.group_lines_device(*batch, parts[0], max_keys=mk, stream=st),
         lambda: g.group_sessions_device(*batch, parts, SESSIONS_GAP, max_sessions=n, max_entries=n, stream=st, **key_outs, **sptrs),
         lambda: g.group_sessions_device(*batch, parts, SESSIONS_GAP, max_keys=mk, stream=st)]
res = timed(calls)
labels = ["gx_group_windows, every output", "gx_group_windows, size query", "... every output, all digits", "... size query, all digits",
          "... size query, short window (0)", "... size query, whole-run window", "gx_group_lines, size query", "gx_group_sessions, every output (the yardstick)",
          "gx_group_sessions, size query"]
for label, (med, mn) in zip(labels, res):
    say("    %-48s %9.3f ms (min %.3f)" % (label, med, mn))
say("    the parts of the call, by difference of medians: the build it stands on %.3f ms; keys pass, sorts, window pass, flags, scan, trips %.3f ms; emits %.3f ms"
    % (res[6][0], res[1][0] - res[6][0], res[0][0] - res[1][0]))
say("    size query against gx_group_sessions' (same keys pass and sorts): %+.3f ms; whole-run window against short: %+.3f ms"
    % (res[1][0] - res[8][0], res[5][0] - res[4][0]))
say("    the host path, for scale: download of line_key and the times %.1f ms, numpy lexsort %.1f ms, the deque loop over the first %d entries %.1f ms"
    % (t_down, t_sort, m_deque, t_deque))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
