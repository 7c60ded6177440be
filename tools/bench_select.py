#!/usr/bin/env python3
"""Developer tool: time the outcome calls (gx_count_outcomes, gx_select_lines) on config 2 (README definition, N x 200-byte lines
on the device, u8 result rows): counts only, keep the unmatched lines (2 %), keep GetRequest (45 %), keep everything -- each
next to a plain device-to-device copy_ of a uint8 tensor as large as what the call writes, and next to the extraction step of the
same batch.  Times by events around repeated calls; gx_select_lines synchronises once per call (the host reads the two sizes
between scan and copy), which is part of what a caller pays and so of the time.  Usage: bench_select.py [lines] [line_bytes]"""
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


def extract():
    g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, no_sync=True, line_bytes_hint=lb, max_line_bytes=lb, compact=2)


print("device: %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), n, lb, width))
ms_x, min_x = timed(extract)
print("%-16s %8.3f ms (min %.3f)" % ("extraction", ms_x, min_x))
assert torch.equal(rows[:, 0].view(torch.int8).to(torch.int32), cat.to(torch.int32))
ms, mn = timed(lambda: g.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=st))
print("%-16s %8.3f ms (min %.3f)  %s" % ("counts only", ms, mn, g.count_outcomes_device(rows.data_ptr(), n, compact=2, stream=st).tolist()))
for label, want in (("keep unmatched", "unmatched"), ("keep GetRequest", "GetRequest"),
                    ("keep everything", ["PutRequest", "GetRequest", "OtherRequest", "unmatched", "exceptions"])):
    mask = g.want_mask(want)
    args = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None, mask)
    k, nbytes = g.select_lines_device(*args, compact=2, stream=st)
    out = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    o_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
    o_index = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
    o_rows = torch.empty((max(k, 1), width), dtype=torch.uint8, device="cuda")
    outs = dict(out_index_ptr=o_index.data_ptr(), out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_rows.data_ptr(),
                cap_lines=k, out_bytes_cap=nbytes, compact=2, stream=st)
    ms, mn = timed(lambda: g.select_lines_device(*args, **outs))
    ms_q, _ = timed(lambda: g.select_lines_device(*args, compact=2, stream=st))
    written = nbytes + 4 * k + 4 * (k + 1) + width * k
    src, dst = torch.empty(written, dtype=torch.uint8, device="cuda"), torch.empty(written, dtype=torch.uint8, device="cuda")
    ms_c, _ = timed(lambda: dst.copy_(src))
    print("%-16s %8.3f ms (min %.3f): %d lines, %.3f GB written (text + offsets + index + rows); flags + scan + sizes alone %.3f ms; "
          "copy_ of as many bytes %.3f ms (x%.1f); extraction %.3f ms" % (label, ms, mn, k, written / 1e9, ms_q, ms_c, ms / ms_c, ms_x))
    keep = torch.from_numpy(mask.astype(bool)).cuda()[torch.where(cat >= 0, cat.long(), 3)]
    assert k == int(keep.sum()) and torch.equal(out[:nbytes], data.view(n, lb)[keep].reshape(-1)) and torch.equal(o_rows[:k], rows[keep])
