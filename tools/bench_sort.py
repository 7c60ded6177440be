#!/usr/bin/env python3
"""Developer tool: time gx_sort_lines on N lines of the README definition (gorp_amd/workloads.py, 200 bytes a line), extracted on the
device (int32 ids and dense capture rows), ordered by their timestamp -- nine digits, written here so that the batch is (a) already in
order and (b) two interleaved halves: two files of alternating instants, one behind the other.  Next to it, in the same process on the
same device:
  by key   gx_lines_by_key by path (the parent commit's call): the same copy, the same number of lines, four digits of a 32-bit sort;
  host     the loop the call replaces: ids, capture rows and text come down, the timestamps are read from the rows with numpy, the
           stamped lines' numbers go through np.argsort(kind="stable"), and a numpy gather moves the bytes (fixed-width lines: one fancy
           index over rows of 200 bytes), the ids and the capture rows.
The new call's result is compared with the host loop's before anything is timed.  Every call is timed as a caller pays for it, its own
synchronisations included: device events around each single call, the median and the minimum of R calls behind one warm-up call; host
cases by wall clock.  The per-pass figures are differences between calls that stop at different points (size query: keys, scan,
compaction, entries, totals; index, values and class alone: + the sort's passes, the finish, the scan; everything: + the copy), not
kernel timings.  The two expectations of the call's issue are marked MET or MISSED from these figures.
Usage: bench_sort.py [lines] [--out FILE] [--reps R]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sort_lines.txt")
reps = 7
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--reps" in argv:
    at = argv.index("--reps"); reps = int(argv[at + 1]); del argv[at:at + 2]
n = int(argv[0]) if len(argv) > 0 else 10_000_000
report = []
L = W.LINE_BYTES
STEP = 80                                   # 10 M instants of nine digits


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
say("device: %s; library %s; %d lines x %d bytes of the README definition, int32 ids and dense capture rows" % (
    torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, L))
by_time = g.top_parts([("PutRequest", "timestamp"), ("GetRequest", "timestamp"), ("OtherRequest", "timestamp")])
by_path = g.group_parts([("PutRequest", "path"), ("GetRequest", "path"), ("OtherRequest", "path")])


def stamp(instants):
    """the lines' nine timestamp digits from `instants` (int64 on the device), and the extraction again"""
    rows = data.view(n, L)
    rest = instants.clone()
    for c in range(9, 0, -1):
        rows[:, c] = (48 + rest % 10).to(torch.uint8)
        rest //= 10
    g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), line_bytes_hint=L)
    torch.cuda.synchronize()


def timed(fn, r=None):
    """(median, min) ms of r single calls, behind one warm-up call"""
    r = r or reps
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(r):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


verdicts = []
i64 = torch.arange(n, dtype=torch.int64, device="cuda")
half = (n + 1) // 2
inputs = (("already in order", 100_000_000 + i64 * STEP),
          ("two interleaved halves", 100_000_000 + torch.where(i64 < half, 2 * i64, 2 * (i64 - half) + 1) * STEP))
for name, instants in inputs:
    stamp(instants)
    batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), by_time)
    rc, t = g.sort_lines_device(*batch)
    m, units, passes = t["lines_out"], t["units_out"], t["n_passes"]
    say("")
    say("%s: %d of %d lines have a timestamp, %d six-bit digits differ, already_ordered %d, %d bytes leave" % (name, m, n, passes, t["already_ordered"], units))
    # the parent's call on the same batch: by path, every line its own key
    kb = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr(), by_path)
    rc, tk = g.lines_by_key_device(*kb, max_keys=n)
    k, km, kunits = tk["n_keys"], tk["lines_out"], tk["units_out"]
    kpasses = (max(k - 1, 0).bit_length() + 5) // 6
    assert km == m and kunits == units                                # the same lines leave both calls: the same copy
    o_index, o_values, o_class = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m, dtype=torch.uint8, device="cuda")
    o_data, o_off = torch.empty(units + 16, dtype=torch.uint8, device="cuda"), torch.empty(m + 1, dtype=torch.int32, device="cuda")
    o_ids, o_caps = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty((m, slots), dtype=torch.int32, device="cuda")
    light = dict(out_index_ptr=o_index.data_ptr(), out_values_ptr=o_values.data_ptr(), out_class_ptr=o_class.data_ptr(), cap_lines=m)
    full = dict(light, out_data_ptr=o_data.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(), out_caps_ptr=o_caps.data_ptr(), out_bytes_cap=units)

    # the host loop, and the result checked against it
    def host_loop():
        h_data, h_ids, h_caps = data.cpu().numpy(), ids.cpu().numpy(), caps.cpu().numpy()
        lines = np.flatnonzero(h_ids >= 0)
        stamps = (h_data.reshape(n, L)[lines, 1:10].astype(np.int64) - 48) @ (10 ** np.arange(8, -1, -1, dtype=np.int64))
        order = lines[np.argsort(stamps, kind="stable")]
        return h_data, h_ids, h_caps, stamps, order
    t_host, (h_data, h_ids, h_caps, stamps, order) = wall(host_loop)
    t_gather, gathered = wall(lambda: (h_data.reshape(n, L)[order].reshape(-1), h_ids[order], h_caps[order]))
    g.sort_lines_device(*batch, stream=st, **full)
    torch.cuda.synchronize()
    assert m == len(order) and np.array_equal(o_index.cpu().numpy().view(np.uint32), order.astype(np.uint32)) and np.array_equal(o_data[:units].cpu().numpy(), gathered[0])
    assert np.array_equal(o_ids.cpu().numpy(), gathered[1]) and np.array_equal(o_caps.cpu().numpy(), gathered[2]) and not o_class.any()
    assert np.array_equal(o_values.cpu().numpy(), np.sort(stamps, kind="stable")) and np.array_equal(o_off.cpu().numpy(), np.arange(m + 1, dtype=np.int32) * L)
    del gathered
    say("  result equals the host loop's (timestamps read from the rows, stable argsort, numpy gather)")
    q = timed(lambda: g.sort_lines_device(*batch, stream=st))
    idx = timed(lambda: g.sort_lines_device(*batch, stream=st, **light))
    ful = timed(lambda: g.sort_lines_device(*batch, stream=st, **full))
    all_idx = timed(lambda: g.sort_lines_device(*batch, stream=st, all_digits=True, **light))
    kol, kou = torch.empty(k + 1, dtype=torch.int64, device="cuda"), torch.empty(k + 1, dtype=torch.int64, device="cuda")
    klight = dict(out_index_ptr=o_index.data_ptr(), cap_lines=km, key_out_lines_ptr=kol.data_ptr(), key_out_units_ptr=kou.data_ptr())
    kfull = dict(klight, out_data_ptr=o_data.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(), out_caps_ptr=o_caps.data_ptr(), out_bytes_cap=kunits)
    kq = timed(lambda: g.lines_by_key_device(*kb, max_keys=n, stream=st))
    kidx = timed(lambda: g.lines_by_key_device(*kb, max_keys=n, stream=st, **klight))
    kful = timed(lambda: g.lines_by_key_device(*kb, max_keys=n, stream=st, **kfull))
    say("  device arrays, ms per call, median (min) of %d calls:" % reps)
    say("    gx_sort_lines, size query                       %9.3f (%9.3f)" % q)
    say("    gx_sort_lines, index, values and class alone    %9.3f (%9.3f)   %d sort passes, finish, scan: +%.3f" % (idx + (passes, idx[0] - q[0])))
    say("    gx_sort_lines, every output                     %9.3f (%9.3f)   the copy of %d bytes and %d rows: +%.3f" % (ful + (units, m, ful[0] - idx[0])))
    say("    gx_sort_lines, index ... alone, all 11 digits   %9.3f (%9.3f)" % all_idx)
    say("    gx_lines_by_key by path, size query             %9.3f (%9.3f)   %d keys" % (kq + (k,)))
    say("    gx_lines_by_key by path, index and bounds alone %9.3f (%9.3f)   emit, compaction, %d sort passes, scan, bounds: +%.3f" % (kidx + (kpasses, kidx[0] - kq[0])))
    say("    gx_lines_by_key by path, every output           %9.3f (%9.3f)   the same copy: +%.3f" % (kful + (kful[0] - kidx[0],)))
    say("  host arrays, ms (wall clock, once):")
    say("    rows and text down, timestamps, stable argsort  %9.1f" % t_host)
    say("    numpy gather of bytes, ids and rows             %9.1f   host loop in all: %.1f" % (t_gather, t_host + t_gather))
    # 1. the cost per sort pass against gx_lines_by_key's same figure
    k_med, k_min = (kidx[0] - kq[0]) / max(kpasses, 1), (kidx[1] - kq[1]) / max(kpasses, 1)
    spread = abs(k_med - k_min)
    bound = 1.6 * k_med + spread
    if passes:
        per = (idx[0] - q[0]) / passes
        verdicts.append("1. cost per sort pass, %s: %.3f ms (%d passes) against 1.6 x %.3f + %.3f = %.3f ms of gx_lines_by_key by path (%d passes): %s" % (
            name, per, passes, k_med, spread, bound, kpasses, "MET" if per <= bound else "MISSED"))
    else:
        per11 = (all_idx[0] - q[0]) / 11
        verdicts.append("1. cost per sort pass, %s: the plan has no pass; with all 11 digits %.3f ms a pass against 1.6 x %.3f + %.3f = %.3f ms of "
                        "gx_lines_by_key by path (%d passes): %s" % (name, per11, k_med, spread, bound, kpasses, "MET" if per11 <= bound else "MISSED"))
    # 2. every output against the host loop
    host_all = t_host + t_gather
    verdicts.append("2. every output, %s: %.3f ms against the host loop's %.1f ms, a factor of %.0f: %s" % (
        name, ful[0], host_all, host_all / ful[0], "MET" if ful[0] < host_all else "MISSED"))
    del h_data, h_ids, h_caps, o_data, o_caps

say("")
say("the two expectations:")
for v in verdicts:
    say("  " + v)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
