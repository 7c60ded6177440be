#!/usr/bin/env python3
"""Developer tool: time gx_group_lines on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) in three cases
  (a) key = the verb of all three extractions: six keys, every matched line keyed -- the contended case;
  (b) the same with value timeTakenInMsec: a gx_measure_stats per key;
  (c) key = the path of all three extractions: long, nearly every line its own key -- the table's case;
each next to, in the same process and alternating round by round, gx_capture_stats with one measure per extraction on timeTakenInMsec:
the yardstick from before gx_group_lines existed -- the same row, offset and value loads and the same parse.  The bound, stated before
anything was measured: (a) and (b) take no more than twice that gx_capture_stats.  (c) carries no bound; printed beside it are the
table's memory and the claims per microsecond.  Every case is timed as the full call (keys, rows and line_key written to device
buffers) and as the size query (build, flags and scans alone).  Times by events around repeated calls; every call synchronises once,
which is part of what a caller pays.  GX_BENCH_LIB names another build of the library (build.py --variant nolds -DGX_GROUP_NO_LDS: the
build pass without the workgroup's LDS table).
Usage: bench_group.py [lines] [line_bytes] [--out FILE] [--append] [--cases abc]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_lines.txt")
append, cases = False, "abc"
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--append" in argv:
    argv.remove("--append"); append = True
if "--cases" in argv:
    at = argv.index("--cases"); cases = argv[at + 1]; del argv[at:at + 2]
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
measures = g.measures([(name, "timeTakenInMsec") for name in names])


def timed_pair(calls, reps=5, rounds=7):
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


def case(label, parts, max_keys, units_cap, values, bound):
    parts = g.group_parts(parts)
    units = torch.empty(max(1, units_cap), dtype=torch.uint8, device="cuda")
    koff = torch.empty(max_keys + 1, dtype=torch.int32, device="cuda")
    first = torch.empty(max_keys, dtype=torch.int32, device="cuda")
    lines = torch.empty(max_keys, dtype=torch.int64, device="cuda")
    stats = torch.empty((max_keys, 8), dtype=torch.int64, device="cuda") if values else None
    lkey = torch.empty(n, dtype=torch.int32, device="cuda")
    full = lambda: g.group_lines_device(*batch, parts, key_units_ptr=units.data_ptr(), key_units_cap=units_cap, key_offsets_ptr=koff.data_ptr(),
                                        key_first_line_ptr=first.data_ptr(), key_lines_ptr=lines.data_ptr(), key_stats_ptr=stats.data_ptr() if values else None,
                                        line_key_ptr=lkey.data_ptr(), max_keys=max_keys, compact=2, stream=st)
    query = lambda: g.group_lines_device(*batch, parts, max_keys=max_keys, compact=2, stream=st)
    yard = lambda: g.capture_stats_device(*batch, measures, compact=2, stream=st)
    rc, totals = full()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["exact"] and totals["lines"] == totals["keyed"] == int((cat >= 0).sum()), (rc, totals)
    whole = yard()
    assert sum(s["lines"] for s in whole) == totals["lines"] and int(lines[:totals["n_keys"]].sum()) == totals["lines"]
    if values:   # the keys' numbers add up to the extractions'
        assert int(stats[:totals["n_keys"], 1].sum()) == sum(s["numbers"] for s in whole) and int(stats[:totals["n_keys"], 6].sum()) == sum(s["sum"] for s in whole)
    (ms_full, mn_full), (ms_query, mn_query), (ms_yard, mn_yard) = timed_pair([full, query, yard])
    say("(%s) %s: %d keys of %d units over %d lines" % (label, ", ".join("%s.%s%s" % (names[parts.array[t].extraction], "verb" if parts.array[t].key_group == 1 else "path",
                                                                                 " + timeTakenInMsec" if parts.array[t].value_group >= 0 else "")
                                                                    for t in range(parts.n)), totals["n_keys"], totals["key_units"], totals["lines"]))
    say("    gx_group_lines, every output          %8.3f ms (min %.3f)" % (ms_full, mn_full))
    say("    gx_group_lines, size query            %8.3f ms (min %.3f)" % (ms_query, mn_query))
    say("    gx_capture_stats, 3 measures          %8.3f ms (min %.3f)" % (ms_yard, mn_yard))
    say("    group_lines / capture_stats = %.2f (every output), %.2f (size query)%s" % (ms_full / ms_yard, ms_query / ms_yard,
                                                                                        "; the bound: 2.00 -- %s" % ("held" if ms_full <= 2 * ms_yard else "MISSED") if bound else "; no bound"))
    return totals, ms_full, ms_query


verb = [(name, "verb") for name in names]
if "a" in cases:
    case("a", verb, 64, 1024, False, True)
if "b" in cases:
    case("b", [(name, "verb", "timeTakenInMsec") for name in names], 64, 1024, True, True)
if "c" in cases:
    totals, ms_full, ms_query = case("c", [(name, "path") for name in names], n, n * lb, False, False)
    slots = 64
    while slots < 2 * n:
        slots *= 2
    say("    table: %d slots x 24 B (slot word, lines, first line) + 4 B key number = %.0f MB; per-line arrays %.0f MB" % (slots, slots * 28 / 1e6, n * 25 / 1e6))
    say("    %d claims (one compare-and-swap per key) in the size query's %.3f ms: %.1f per us over the whole table (one word takes about 88 returning atomics per us)"
        % (totals["n_keys"], ms_query, totals["n_keys"] / ms_query / 1e3))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(report) + "\n")
