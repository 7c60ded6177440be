#!/usr/bin/env python3
"""Developer tool: time gx_partition_lines on config 2 (README definition, N x 200-byte lines on the device, u8 result rows, four
non-empty outcomes), on config 3's batch (64 syslog-like extractions, a 100 000-line sample tiled to N lines, u8 result rows) and
on a short-line batch (--config 0: N lines of 4 .. 28 random bytes, synthetic int32 ids over four outcomes of the README
definition: nearly every 16-byte chunk of the output holds a line boundary there).
Each batch alternates, in this one process:
  (a) one gx_partition_lines that writes text, offsets, line numbers and rows;
  (b) what there was before it: one gx_select_lines per non-empty outcome with the same outputs, each into its slice of the same
      buffers (the non-empty outcomes and the slices are worked out before the clock starts);
  (c) a plain device-to-device copy_ of a uint8 tensor as large as what (a) writes.
Times by events around repeated calls; both calls synchronise once per call (the host reads the sizes between scan and copy),
which is part of what a caller pays and so of the time.  The output of (b) is compared with (a)'s before anything is timed.
Usage: bench_partition.py [lines] [--config 0|2|3] [--once]      (--once: three partitions per batch and nothing else: the run to put
under rocprofv3 --kernel-trace --stats for the per-kernel times)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

args_in = sys.argv[1:]
once = "--once" in args_in
configs = [2, 3, 0]
if "--config" in args_in:
    at = args_in.index("--config")
    configs = [int(args_in[at + 1])]
    del args_in[at:at + 2]
rest = [a for a in args_in if not a.startswith("--")]
n_arg = int(rest[0]) if rest else 10_000_000
st = torch.cuda.current_stream().cuda_stream


def timed(call, reps, rounds=5):
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


def workload(config):
    """(handle, code units, offsets, lines, ids or None = extract u8 rows here, description)"""
    if config == 2:
        g = Gorp.construct(W.readme3_definition())
        data, off, _ = W.readme3_lines(n_arg, seed=2, device="cuda")
        return g, data, off.to(torch.int64).to(torch.int32), n_arg, None, "config 2: README definition, %d x %d B lines" % (n_arg, W.LINE_BYTES)
    if config == 0:
        g = Gorp.construct(W.readme3_definition())
        gen = torch.Generator(device="cuda").manual_seed(5)
        lens = torch.randint(4, 29, (n_arg,), device="cuda", generator=gen, dtype=torch.int64)
        off = torch.cat([torch.zeros(1, device="cuda", dtype=torch.int64), lens.cumsum(0)]).to(torch.int32)
        data = torch.randint(32, 127, (int(off[-1]),), device="cuda", generator=gen, dtype=torch.uint8)
        ids = (torch.randint(0, 4, (n_arg,), device="cuda", generator=gen, dtype=torch.int32) - 1).contiguous()   # -1, 0, 1, 2
        return g, data, off, n_arg, ids, "short lines: %d lines of 4 .. 28 B (mean %.1f), synthetic int32 ids" % (n_arg, float(off[-1]) / n_arg)
    rules, meta = W.syslog_definition(64, seed=3)
    base_n = 100_000
    dh, oh, _ = W.syslog_lines(meta, base_n, seed=3)
    total, reps = int(oh[-1]), max(1, n_arg // base_n)
    while total * reps >= 2 ** 31:
        reps -= 1
    data = torch.from_numpy(dh.copy()).cuda().repeat(reps)
    off = (torch.from_numpy(oh[:-1].astype(np.int64)).cuda()[None, :] + torch.arange(reps, device="cuda", dtype=torch.int64)[:, None] * total).reshape(-1)
    off = torch.cat([off, torch.tensor([total * reps], device="cuda", dtype=torch.int64)]).to(torch.int32)
    return Gorp.construct(rules), data, off, base_n * reps, None, "config 3: 64 syslog-like extractions, %d uneven lines, mean %.1f B (a %d-line sample tiled)" % (
        base_n * reps, total / base_n, base_n)


print("device: %s" % torch.cuda.get_device_name(0))
for config in configs:
    g, data, off, n, rows, desc = workload(config)
    K = g.num_extractions
    if rows is None:
        compact, width, what = 2, 1 + 2 * g.max_groups, "u8 result rows of %d bytes" % (1 + 2 * g.max_groups)
        rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
        g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=200, compact=2)
    else:
        compact, width, what = 0, 4, "int32 ids, no capture rows"
    args = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)
    k, nbytes, group_lines, group_units = g.partition_lines_device(*args, None, compact=compact, stream=st)
    gl, gu = group_lines.astype(np.int64), group_units.astype(np.int64)
    nonempty = [x for x in range(2 * K + 1) if gl[x + 1] > gl[x]]
    print("%s, %s; %d of %d lines kept, %d non-empty outcomes, %d sort digit(s)" % (
        desc, what, k, n, len(nonempty), -(-int(2 * K + 1).bit_length() // 6)))

    def buffers():
        return (torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda"), torch.empty(k + 1, dtype=torch.int32, device="cuda"),
                torch.empty(max(k, 1), dtype=torch.int32, device="cuda"), torch.empty(max(k, 1) * width, dtype=torch.uint8, device="cuda"))

    out, o_off, o_index, o_rows = buffers()

    def partition():
        g.partition_lines_device(*args, None, out_index_ptr=o_index.data_ptr(), out_data_ptr=out.data_ptr(), out_offsets_ptr=o_off.data_ptr(),
                                 out_ids_ptr=o_rows.data_ptr(), cap_lines=k, out_bytes_cap=nbytes, compact=compact, stream=st)

    if once:
        for _ in range(3):
            partition()
        torch.cuda.synchronize()
        continue
    s_out, s_off, s_index, s_rows = buffers()
    s_off_scratch = torch.empty(k + 1 + len(nonempty), dtype=torch.int32, device="cuda")   # (every selection's offsets start at 0: one array each)
    masks, at = [], 0
    for x in nonempty:
        m = np.zeros(2 * K + 1, np.uint8)
        m[x] = 1
        lines, units = int(gl[x + 1] - gl[x]), int(gu[x + 1] - gu[x])
        masks.append((m, dict(out_index_ptr=s_index.data_ptr() + 4 * int(gl[x]), out_data_ptr=s_out.data_ptr() + int(gu[x]),
                              out_offsets_ptr=s_off_scratch.data_ptr() + 4 * at, out_ids_ptr=s_rows.data_ptr() + width * int(gl[x]),
                              cap_lines=lines, out_bytes_cap=units, compact=compact, stream=st)))
        at += lines + 1

    def selects():
        for m, outs in masks:
            g.select_lines_device(*args, m, **outs)

    partition(); selects(); torch.cuda.synchronize()
    assert torch.equal(out, s_out) and torch.equal(o_index, s_index) and torch.equal(o_rows, s_rows)
    written = nbytes + 4 * k + 4 * (k + 1) + width * k
    src, dst = torch.empty(written, dtype=torch.uint8, device="cuda"), torch.empty(written, dtype=torch.uint8, device="cuda")
    reps_b = 3 if len(nonempty) > 8 else 10
    ms_a, min_a = timed(partition, 10)
    ms_b, min_b = timed(selects, reps_b)
    ms_c, min_c = timed(lambda: dst.copy_(src), 10)
    ms_a2, min_a2 = timed(partition, 10)   # (a) again, behind (b) and (c): the order of the runs is not what is measured
    ms_q, _ = timed(lambda: g.partition_lines_device(*args, None, compact=compact, stream=st), 10)
    print("  (a) one gx_partition_lines          %8.3f ms (min %.3f); again at the end %.3f ms (min %.3f); keys + sort + scan + sizes alone %.3f ms" % (
        ms_a, min_a, ms_a2, min_a2, ms_q))
    print("  (b) %3d gx_select_lines             %8.3f ms (min %.3f)" % (len(nonempty), ms_b, min_b))
    print("  (c) copy_ of the %.3f GB (a) writes %8.3f ms (min %.3f)" % (written / 1e9, ms_c, min_c))
    print("  (a)/(b) = %.3f   (a)/(c) = %.2f" % (max(ms_a, ms_a2) / ms_b, max(ms_a, ms_a2) / ms_c))
    del src, dst, s_out, s_off, s_index, s_rows, out, o_off, o_index, o_rows, rows, data, off
    torch.cuda.empty_cache()
