#!/usr/bin/env python3
"""Developer tool: time gx_select_lines_where on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) next
to gx_select_lines on the same batch in the same run, with a mask that keeps a like share of the lines:
  (a) GetRequest: timeTakenInMsec >= T    T = 0 keeps every GetRequest line -- exactly what the mask "GetRequest" keeps, byte for byte;
                                          T = 500 keeps a third of them, next to the mask "OtherRequest + unmatched"
  (b) OtherRequest: verb == "GET"         keeps nothing (GetRequest comes first), next to the empty mask
  (c) GetRequest: path contains "/v1/"    a scan of a 170-byte value per line that keeps next to nothing, next to the empty mask
For each: the whole call with every output, the size query alone (flags + scan + the host's read of the sizes; the difference between the
two calls' size queries is the difference between their flags passes), and the algorithmic bytes of the flags pass -- id and row, two
offsets per line, and the code units of the tested values.  Times by events around repeated calls; either call synchronises once per
call, which is part of what a caller pays.  Usage: bench_where.py [lines] [line_bytes]"""
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


def buffers(k, nbytes):
    out = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    o_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
    o_index = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
    o_rows = torch.empty((max(k, 1), width), dtype=torch.uint8, device="cuda")
    return (out, o_off, o_index, o_rows), dict(out_index_ptr=o_index.data_ptr(), out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(),
                                               out_ids_ptr=o_rows.data_ptr(), cap_lines=k, out_bytes_cap=nbytes, compact=2, stream=st)


def run_select(want):
    mask = g.want_mask(want)
    args = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None, mask)
    k, nbytes = g.select_lines_device(*args, compact=2, stream=st)
    keepalive, outs = buffers(k, nbytes)
    ms, mn = timed(lambda: g.select_lines_device(*args, **outs))
    ms_q, _ = timed(lambda: g.select_lines_device(*args, compact=2, stream=st))
    return dict(ms=ms, min=mn, query=ms_q, k=k, nbytes=nbytes, out=keepalive)


def run_where(spec, want="matched-by-terms"):
    w = g.where_terms(spec)
    mask = g._where_want(w, want)
    args = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None, mask, w)
    k, nbytes = g.select_lines_where_device(*args, compact=2, stream=st)
    keepalive, outs = buffers(k, nbytes)
    ms, mn = timed(lambda: g.select_lines_where_device(*args, **outs))
    ms_q, _ = timed(lambda: g.select_lines_where_device(*args, compact=2, stream=st))
    # the flags pass's algorithmic bytes: a row and two offsets per line, and the tested values of the lines whose extraction has terms
    value_units = 0
    for t in list(w.array)[:w.n]:
        of_k = rows[:, 0].view(torch.int8) == t.extraction
        b, e = rows[of_k, 1 + 2 * t.group].long(), rows[of_k, 2 + 2 * t.group].long()
        value_units += int((e - b).sum())
    return dict(ms=ms, min=mn, query=ms_q, k=k, nbytes=nbytes, out=keepalive, flag_bytes=n * (width + 8) + value_units, value_units=value_units)


def check(res, keep):
    out, o_off, o_index, o_rows = res["out"]
    assert res["k"] == int(keep.sum()) and torch.equal(out[:res["nbytes"]], data.view(n, lb)[keep].reshape(-1)) and torch.equal(o_rows[:res["k"]], rows[keep])


is_get = cat == names.index("GetRequest")
# timeTakenInMsec of the generator's lines: the digits between the verb's blank and "ms" (workloads.readme3_lines)
cases = [("(a) GetRequest timeTakenInMsec >= 0", [("GetRequest", "timeTakenInMsec", ">=", 0)], "GetRequest"),
         ("(a) GetRequest timeTakenInMsec >= 500", [("GetRequest", "timeTakenInMsec", ">=", 500)], ["OtherRequest", "unmatched"]),
         ("(b) OtherRequest verb == \"GET\"", [("OtherRequest", "verb", "==", "GET")], []),
         ("(c) GetRequest path contains \"/v1/\"", [("GetRequest", "path", "contains", "/v1/")], [])]
yard = {}
for label, spec, like in cases:
    key = str(like)
    if key not in yard:
        yard[key] = run_select(like)
    s, w = yard[key], run_where(spec)
    if ">= 0" in label:
        check(w, is_get)
        check(s, is_get)
    print("%s" % label)
    print("    gx_select_lines_where %8.3f ms (min %.3f): %d lines kept (%.1f %%), %.3f GB of text; size query alone %.3f ms; flags pass reads %.3f GB "
          "(%.3f GB of values)" % (w["ms"], w["min"], w["k"], 100.0 * w["k"] / n, w["nbytes"] / 1e9, w["query"], w["flag_bytes"] / 1e9, w["value_units"] / 1e9))
    print("    gx_select_lines       %8.3f ms (min %.3f): %d lines kept (%.1f %%), %.3f GB of text; size query alone %.3f ms; mask %s"
          % (s["ms"], s["min"], s["k"], 100.0 * s["k"] / n, s["nbytes"] / 1e9, s["query"], like or "empty"))
    print("    where / select = %.3f; size queries %.3f - %.3f = %.3f ms more in the flags pass; copy pass (call - query) %.3f ms against %.3f ms"
          % (w["ms"] / s["ms"], w["query"], s["query"], w["query"] - s["query"], w["ms"] - w["query"], s["ms"] - s["query"]))
