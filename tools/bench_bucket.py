#!/usr/bin/env python3
"""Developer tool: time gx_bucket_lines on config 2 (README definition, N x 200-byte lines on the device, u8 result rows), the lines'
nine-digit timestamps rewritten in place (the result rows hold offsets alone and stay valid) into three shapes
  (a) time-ordered, timestamp = line number, about 20 buckets: ten million lines fall into a handful of buckets -- the contended case;
  (b) time-ordered, about 15 000 buckets;
  (c) shuffled, every line its own bucket -- the table's and the sort's case;
each next to, in the same process and alternating round by round, gx_group_lines on the same batch keyed by `verb` (6 keys): the yardstick,
code this call does not touch.  The expectation for (a), stated before anything was measured: gx_bucket_lines does the same pass plus a
parse and minus a text compare, so its median should not exceed gx_group_lines' median by more than that run's own min-to-median spread.
(b) and (c) carry no bound.  Every shape is timed as the full call (bucket_number, first line, lines and line_bucket written to device
buffers) and as the size query (build, flags and scan alone).  Times by events around repeated calls after a warm-up, median and minimum
over the rounds; every call synchronises once, which is part of what a caller pays.  Beside them the host alternative available without
the call: a download of the result rows and the text and a Python loop (int(), //, a dict) -- timed once, on the first --host-lines lines.
Usage: bench_bucket.py [lines] [line_bytes] [--out FILE] [--append] [--cases abc] [--host-lines M]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bucket_lines.txt")
append, cases, host_lines = False, "abc", 1_000_000
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--append" in argv:
    argv.remove("--append"); append = True
if "--cases" in argv:
    at = argv.index("--cases"); cases = argv[at + 1]; del argv[at:at + 2]
if "--host-lines" in argv:
    at = argv.index("--host-lines"); host_lines = int(argv[at + 1]); del argv[at:at + 2]
n = int(argv[0]) if len(argv) > 0 else 10_000_000
lb = int(argv[1]) if len(argv) > 1 else W.LINE_BYTES
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


g = Gorp.construct(W.readme3_definition())
names = [x.getName() for x in g.getExtractions()]
data, off, cat = W.readme3_lines(n, seed=2, device="cuda", line_bytes=lb)
width = 1 + 2 * g.max_groups
rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
g.extract_batch_device(data.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb, max_line_bytes=lb, compact=2)
torch.cuda.synchronize()
assert torch.equal(rows[:, 0].view(torch.int8).to(torch.int32), cat.to(torch.int32))
say("device: %s; library %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, lb, width))
batch = (data.data_ptr(), off.data_ptr(), n, rows.data_ptr(), None)
matched = int((cat >= 0).sum())
assert n <= 10 ** 9
verb_parts = g.group_parts([(name, "verb") for name in names])
ts_parts = g.bucket_parts([(name, "timestamp") for name in names])


def stamp(ts):
    """the lines' timestamps: ts[i] in nine digits, zero-padded, in place"""
    view = data.view(n, lb)
    q = ts.clone()
    for d in range(9, 0, -1):
        view[:, d] = (48 + q % 10).to(torch.uint8)
        q //= 10
    torch.cuda.synchronize()


def timed(calls, reps=5, rounds=7):
    """median and minimum ms per call of every call in `calls`, the calls taking turns round by round"""
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need 25 ms of unbroken load: profiles/r04_clock_ramp.txt)
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
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def host_alternative(bucket_width):
    """the downloads and the loop on the first m lines: seconds of wall clock for each step"""
    m = min(n, host_lines)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h_rows, h_data = rows[:m].cpu().numpy(), data[:m * lb].cpu().numpy()
    t1 = time.perf_counter()
    per, raw = {}, h_data.tobytes()
    for i, r in enumerate(h_rows.tolist()):
        if r[0] < 128 and r[1] != 0xFF:
            b = int(raw[i * lb + r[1]:i * lb + r[2]]) // bucket_width
            per[b] = per.get(b, 0) + 1
    t2 = time.perf_counter()
    return m, len(per), t1 - t0, t2 - t1


def case(label, what, bucket_width, max_buckets, bound):
    number = torch.empty(max_buckets, dtype=torch.int64, device="cuda")
    first = torch.empty(max_buckets, dtype=torch.int32, device="cuda")
    lines = torch.empty(max_buckets, dtype=torch.int64, device="cuda")
    lbucket = torch.empty(n, dtype=torch.int32, device="cuda")
    units = torch.empty(1024, dtype=torch.uint8, device="cuda")
    koff = torch.empty(65, dtype=torch.int32, device="cuda")
    kfirst = torch.empty(64, dtype=torch.int32, device="cuda")
    klines = torch.empty(64, dtype=torch.int64, device="cuda")
    lkey = torch.empty(n, dtype=torch.int32, device="cuda")
    full = lambda: g.bucket_lines_device(*batch, ts_parts, bucket_width, bucket_number_ptr=number.data_ptr(), bucket_first_line_ptr=first.data_ptr(),
                                         bucket_lines_ptr=lines.data_ptr(), line_bucket_ptr=lbucket.data_ptr(), max_buckets=max_buckets, compact=2, stream=st)
    query = lambda: g.bucket_lines_device(*batch, ts_parts, bucket_width, max_buckets=max_buckets, compact=2, stream=st)
    yard = lambda: g.group_lines_device(*batch, verb_parts, key_units_ptr=units.data_ptr(), key_units_cap=1024, key_offsets_ptr=koff.data_ptr(),
                                        key_first_line_ptr=kfirst.data_ptr(), key_lines_ptr=klines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=64, compact=2,
                                        stream=st)
    yard_query = lambda: g.group_lines_device(*batch, verb_parts, max_keys=64, compact=2, stream=st)
    rc, totals = full()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["exact"] and totals["lines"] == totals["bucketed"] == matched, (rc, totals)
    k = totals["n_buckets"]
    assert int(lines[:k].sum()) == matched and bool((torch.diff(number[:k]) > 0).all()) and int(number[0]) == totals["first_bucket"]
    assert bool(((lbucket == -1) == (cat < 0)).all())
    rc, alone = yard()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and alone["n_keys"] == 6 and alone["lines"] == matched
    (ms_full, mn_full), (ms_query, mn_query), (ms_yard, mn_yard), (ms_yq, mn_yq) = timed([full, query, yard, yard_query])
    say("(%s) %s, width %d: %d buckets (%d .. %d) over %d lines" % (label, what, bucket_width, k, totals["first_bucket"], totals["last_bucket"], matched))
    say("    gx_bucket_lines, every output         %8.3f ms (min %.3f)" % (ms_full, mn_full))
    say("    gx_bucket_lines, size query           %8.3f ms (min %.3f)" % (ms_query, mn_query))
    say("    gx_group_lines by verb, every output  %8.3f ms (min %.3f)" % (ms_yard, mn_yard))
    say("    gx_group_lines by verb, size query    %8.3f ms (min %.3f)" % (ms_yq, mn_yq))
    spread = ms_yard - mn_yard
    say("    bucket_lines / group_lines = %.2f (every output), %.2f (size query)%s"
        % (ms_full / ms_yard, ms_query / ms_yq,
           "; the expectation: no more than gx_group_lines' median plus its min-to-median spread, %.3f + %.3f ms -- %s"
           % (ms_yard, spread, "MET" if ms_full <= ms_yard + spread else "MISSED") if bound else "; no bound"))
    m, found, s_down, s_loop = host_alternative(bucket_width)
    say("    the host alternative on the first %d lines: downloads %.1f ms, a Python loop over %d buckets %.1f ms: %.1f ms, %.0f ns a line"
        % (m, s_down * 1e3, found, s_loop * 1e3, (s_down + s_loop) * 1e3, (s_down + s_loop) * 1e9 / m))
    if m == n:
        assert found == k
    return totals, ms_full, ms_query


line_number = torch.arange(n, dtype=torch.int64, device="cuda")
if "a" in cases or "b" in cases:
    stamp(line_number)
if "a" in cases:
    case("a", "time-ordered", max(1, n // 20), 64, True)
if "b" in cases:
    case("b", "time-ordered", max(1, n // 15000), 1 << 15, False)
if "c" in cases:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    stamp(torch.randperm(n, device="cuda", generator=gen))
    totals, ms_full, ms_query = case("c", "shuffled, every line its own bucket", 1, n, False)
    slots = 64
    while slots < 2 * n:
        slots *= 2
    say("    table: %d slots x 29 B (slot word, lines, first line, scan, rank, flag) = %.0f MB; per line 4 B = %.0f MB; the sort 24 B a bucket = %.0f MB"
        % (slots, slots * 29 / 1e6, n * 4 / 1e6, totals["n_buckets"] * 24 / 1e6))
    say("    %d claims (one compare-and-swap per bucket) in the size query's %.3f ms: %.1f per us over the whole table" % (totals["n_buckets"], ms_query, totals["n_buckets"] / ms_query / 1e3))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(report) + "\n")
