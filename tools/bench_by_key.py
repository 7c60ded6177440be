#!/usr/bin/env python3
"""Developer tool: time gx_lines_by_key on N lines of the README definition (gorp_amd/workloads.py, 200 bytes a line), extracted on the
device (int32 ids and dense capture rows), by verb -- a handful of keys, one digit of the sort -- and by path.  Next to it, in the same
process on the same device, what a caller has without the call:
  device   gx_group_lines with line_key on the device arrays: as far as the family went; the regrouping itself is then still to do;
  host     gx_group_lines on host arrays (line_key comes down), np.argsort(kind="stable") of the keyed lines' key numbers, and a numpy
           gather of the bytes (fixed-width lines: one fancy index over rows of 200 bytes), the ids and the capture rows.
The new call's result is compared with the host loop's before anything is timed.  Every call is timed as a caller pays for it, its own
synchronisations included.  Device cases: events around repeated calls; host cases: wall clock.  The per-pass figures are differences
between calls that stop at different points (size query: build and kept pass; index and bounds alone: + compaction, sort, scan, bounds;
everything: + the copy), not kernel timings.
Usage: bench_by_key.py [lines] [--out FILE] [--reps R]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "by_key.txt")
reps = 5
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--reps" in argv:
    at = argv.index("--reps"); reps = int(argv[at + 1]); del argv[at:at + 2]
n = int(argv[0]) if len(argv) > 0 else 10_000_000
report = []
L = W.LINE_BYTES


def say(line):
    print(line, flush=True)
    report.append(line)


g = Gorp.construct(W.readme3_definition())
slots = 2 * g.max_groups
st = torch.cuda.current_stream().cuda_stream
data, _, _ = W.readme3_lines(n, seed=11, device="cuda")
off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * L).to(torch.int32)
ids = torch.empty(n, dtype=torch.int32, device="cuda")
caps = torch.empty((n, slots), dtype=torch.int32, device="cuda")
g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), line_bytes_hint=L)
torch.cuda.synchronize()
say("device: %s; library %s; %d lines x %d bytes of the README definition, int32 ids and dense capture rows" % (
    torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, L))
h_data, h_off, h_ids, h_caps = data.cpu().numpy(), off.cpu().numpy().view(np.uint32), ids.cpu().numpy(), caps.cpu().numpy()


def timed(fn, r=reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(r):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / r


def wall(fn, r=1):
    t = time.perf_counter()
    for _ in range(r):
        out = fn()
    return (time.perf_counter() - t) * 1e3 / r, out


for name, parts in (("verb", [("PutRequest", "verb"), ("GetRequest", "verb"), ("OtherRequest", "verb")]),
                    ("path", [("PutRequest", "path"), ("GetRequest", "path"), ("OtherRequest", "path")])):
    parts = g.group_parts(parts)
    batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), parts)
    rc, t = g.lines_by_key_device(*batch, max_keys=n)
    k, m, units = t["n_keys"], t["lines_out"], t["units_out"]
    passes = (max(k - 1, 0).bit_length() + 5) // 6
    say("")
    say("by %s: %d keys (%d six-bit digits), %d of %d lines have one, %d bytes kept" % (name, k, passes, m, n, units))
    line_key = torch.empty(n, dtype=torch.int32, device="cuda")
    o_index, o_data, o_off = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(units + 16, dtype=torch.uint8, device="cuda"), torch.empty(m + 1, dtype=torch.int32, device="cuda")
    o_ids, o_caps = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty((m, slots), dtype=torch.int32, device="cuda")
    kol, kou = torch.empty(k + 1, dtype=torch.int64, device="cuda"), torch.empty(k + 1, dtype=torch.int64, device="cuda")
    full = dict(out_index_ptr=o_index.data_ptr(), out_data_ptr=o_data.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(),
                out_caps_ptr=o_caps.data_ptr(), cap_lines=m, out_bytes_cap=units, key_out_lines_ptr=kol.data_ptr(), key_out_units_ptr=kou.data_ptr())
    # the host loop, and the result checked against it
    def host_loop():
        r = g.group_lines(h_data, h_off, h_ids, h_caps, parts, keys="csr", max_keys=n, key_units_cap=64 * k + 64)
        has = r["line_key"] != 0xFFFFFFFF
        return r, np.flatnonzero(has)[np.argsort(r["line_key"][has], kind="stable")]
    t_host, (res, order) = wall(host_loop)
    t_gather, gathered = wall(lambda: (h_data.reshape(n, L)[order].reshape(-1), h_ids[order], h_caps[order]))
    g.lines_by_key_device(*batch, max_keys=n, stream=st, **full)
    torch.cuda.synchronize()
    assert np.array_equal(o_index.cpu().numpy().view(np.uint32), order.astype(np.uint32)) and np.array_equal(o_data[:units].cpu().numpy(), gathered[0])
    assert np.array_equal(o_ids.cpu().numpy(), gathered[1]) and np.array_equal(o_caps.cpu().numpy(), gathered[2])
    assert np.array_equal(kol.cpu().numpy(), np.concatenate([[0], np.cumsum(res["lines"].astype(np.int64))]))
    say("  result equals the host loop's (group_lines, stable argsort of line_key, numpy gather)")
    # device arrays
    t_group_q = timed(lambda: g.group_lines_device(*batch, max_keys=n, stream=st))
    t_group = timed(lambda: g.group_lines_device(*batch, line_key_ptr=line_key.data_ptr(), max_keys=n, stream=st))
    t_q = timed(lambda: g.lines_by_key_device(*batch, max_keys=n, stream=st))
    t_idx = timed(lambda: g.lines_by_key_device(*batch, max_keys=n, stream=st, out_index_ptr=o_index.data_ptr(), cap_lines=m, key_out_lines_ptr=kol.data_ptr(),
                                                key_out_units_ptr=kou.data_ptr()))
    t_full = timed(lambda: g.lines_by_key_device(*batch, max_keys=n, stream=st, **full))
    say("  device arrays, ms per call (%d calls each):" % reps)
    say("    gx_group_lines, size query                      %9.3f" % t_group_q)
    say("    gx_group_lines with line_key (the parent's end) %9.3f   -- the regrouping is then still to do" % t_group)
    say("    gx_lines_by_key, size query                     %9.3f   kept pass, its scan and totals: +%.3f over gx_group_lines' size query" % (t_q, t_q - t_group_q))
    say("    gx_lines_by_key, index and bounds alone         %9.3f   emit, compaction, %d sort passes, scan, bounds: +%.3f" % (t_idx, passes, t_idx - t_q))
    say("    gx_lines_by_key, every output                   %9.3f   the copy of %d bytes and %d rows: +%.3f" % (t_full, units, m, t_full - t_idx))
    # host arrays
    hk = dict(keys="csr", max_keys=n, key_units_cap=64 * k + 64)
    t_new, _ = wall(lambda: g.lines_by_key(h_data, h_off, h_ids, h_caps, parts, **hk))
    say("  host arrays, ms per call (wall clock, one call each):")
    say("    gx_group_lines + stable argsort                 %9.1f" % t_host)
    say("    numpy gather of bytes, ids and rows             %9.1f   host loop in all: %.1f" % (t_gather, t_host + t_gather))
    say("    gx_lines_by_key (Gorp.lines_by_key)             %9.1f" % t_new)

with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
