#!/usr/bin/env python3
"""Developer tool: time gx_group_quantiles on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) asking
p50 / p95 / p99 of timeTakenInMsec, grouped
  (verb) by the verb of all three extractions: six keys, every matched line a candidate;
  (path) by the path of all three extractions: long keys, nearly every line its own;
each next to, in the same process and alternating round by round,
  (a) gx_group_lines alone (the same per-key outputs without the quantiles) and gx_capture_quantiles alone (the same three
      quantiles over the whole batch): their sum is the price of the two questions the library could answer before.  The new call
      does strictly more; the ratio is reported and carries no bound;
  (b) the loop a caller had to write: gx_group_lines once, then one gx_capture_quantiles with an == term per key.  Timed for the verb
      grouping; for the path grouping the loop's cost per key is reported from its first keys and multiplied out, not run.
The new call's rows are compared with (b)'s before anything is timed.  Every call is timed as a caller pays for it: its own
synchronisation included, outputs in device buffers.  Times by events around repeated calls, the calls taking turns round by round.
GX_BENCH_LIB names another build of the library (build.py --variant alldigits -DGX_GQ_ALL_DIGITS: every value digit sorted).
Usage: bench_group_quantiles.py [lines] [line_bytes] [--out FILE] [--append] [--cases verb,path]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_quantiles.txt")
append, cases = False, "verb,path"
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
P = [(50, 100), (95, 100), (99, 100)]
TIME = "timeTakenInMsec"
by_time = g.top_parts([(name, TIME) for name in names])


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


def case(label, key, max_keys, loop_keys):
    """loop_keys: how many keys the loop (b) is run for (None: all of them)"""
    parts = g.group_parts([(name, key, TIME) for name in names])
    koff = torch.empty(max_keys + 1, dtype=torch.int32, device="cuda")
    lines = torch.empty(max_keys, dtype=torch.int64, device="cuda")
    stats = torch.empty((max_keys, 8), dtype=torch.int64, device="cuda")
    kq = torch.empty((max_keys * len(P), 4), dtype=torch.int64, device="cuda")
    out = dict(key_lines_ptr=lines.data_ptr(), key_stats_ptr=stats.data_ptr(), max_keys=max_keys, compact=2, stream=st)
    new = lambda: g.group_quantiles_device(*batch, parts, P, key_quantiles_ptr=kq.data_ptr(), **out)
    keys_only = lambda: g.group_quantiles_device(*batch, parts, P, **out)
    group = lambda: g.group_lines_device(*batch, parts, **out)
    whole = lambda: g.capture_quantiles_device(*batch, by_time, P, compact=2, stream=st)
    rc, totals = new()
    torch.cuda.synchronize()
    k = totals["n_keys"]
    assert rc == N.GX_OK and totals["exact"] and totals["lines"] == totals["keyed"] == int((cat >= 0).sum()), (rc, totals)
    numbers = int(stats[:k, 1].sum())
    assert numbers == whole()[1]["numbers"]
    got = kq[:k * len(P)].view(k, len(P), 4).cpu()
    assert bool((got[:, :, 1] <= stats[:k, 1:2].cpu()).all()) and bool((got[:, :, 2] < got[:, :, 1]).all())
    # the keys' text, for the loop's == terms: the caller's group_lines delivers it (outside the timed window here)
    units = torch.empty(max(1, totals["key_units"]), dtype=torch.uint8, device="cuda")
    rc, _ = g.group_lines_device(*batch, parts, key_units_ptr=units.data_ptr(), key_units_cap=totals["key_units"], key_offsets_ptr=koff.data_ptr(), max_keys=max_keys,
                                 compact=2, stream=st)
    torch.cuda.synchronize()
    assert rc == N.GX_OK
    take = k if loop_keys is None else min(k, loop_keys)
    h_off = koff[:take + 1].cpu().tolist()
    h_units = units[:h_off[take]].cpu().numpy().tobytes()
    texts = [h_units[h_off[j]:h_off[j + 1]] for j in range(take)]
    terms = [g.where_terms([(name, key, "==", t) for name in names]) for t in texts]

    def loop():
        group()
        return [g.capture_quantiles_device(*batch, by_time, P, where=w, compact=2, stream=st)[0] for w in terms]

    for j, res in enumerate(loop()):   # the new call's rows are the loop's
        assert [[r["value"] or 0, r["rank"], r["below"], r["equal"]] for r in res] == got[j].tolist(), (j, res, got[j].tolist())
    (ms_new, mn_new), (ms_keys, mn_keys), (ms_group, mn_group), (ms_whole, mn_whole) = timed([new, keys_only, group, whole])
    say("(%s) p50 / p95 / p99 of %s per %s: %d keys, %d numbers of %d lines" % (label, TIME, key, k, numbers, n))
    say("    gx_group_quantiles, keys + stats + quantiles     %9.3f ms (min %.3f)" % (ms_new, mn_new))
    say("    gx_group_quantiles without key_quantiles         %9.3f ms (min %.3f)" % (ms_keys, mn_keys))
    say("    (a) gx_group_lines, the same per-key outputs     %9.3f ms (min %.3f)" % (ms_group, mn_group))
    say("    (a) gx_capture_quantiles, whole batch            %9.3f ms (min %.3f)" % (ms_whole, mn_whole))
    say("    new / (group_lines + capture_quantiles) = %.2f; the sort and the pick cost %.3f ms over gx_group_lines" % (ms_new / (ms_group + ms_whole), ms_new - ms_group))
    (ms_loop, mn_loop), (ms_again, mn_again) = timed([loop, new], reps=2, rounds=5)
    if take == k:
        say("    (b) gx_group_lines + %d x gx_capture_quantiles(==) %9.3f ms (min %.3f); the new call beside it %.3f ms: %.1f x" % (k, ms_loop, mn_loop, ms_again, ms_loop / ms_again))
        if ms_again > ms_loop:
            say("    THE NEW CALL IS SLOWER THAN THE LOOP")
    else:
        per_key = (ms_loop - ms_group) / take
        say("    (b) not run to its end: %d of its %d gx_capture_quantiles(==) calls take %.3f ms, %.3f ms a key: about %.0f s for all keys against %.3f ms" %
            (take, k, ms_loop - ms_group, per_key, per_key * k / 1e3, ms_again))
    return totals


for c in cases.split(","):
    if c == "verb":
        case("verb", "verb", 64, None)
    elif c == "path":
        case("path", "path", n, 8)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(report) + "\n")
