#!/usr/bin/env python3
"""Developer tool: time gx_group_pairs on config 2 (README definition, N x 200-byte lines on the device, u8 result rows) in three shapes
  (a) verb x verb: as many pairs as keys, six in all, every matched line paired -- the contended case;
  (b) verb x timeTakenInMsec as text: some ten thousand seconds under each verb;
  (c) verb x path: about one pair per line -- the pair table's case;
each next to, in the same process and alternating round by round, gx_group_lines on the same parts and batch: the yardstick, since by
construction the call does the build's work about twice (a second find-or-insert, a second flags / scan / emit).  The expectation,
stated before anything was measured: (a) and (b) land within twice that gx_group_lines.  (c) carries no bound.  Every shape is timed as
the full call (keys, pairs, line_key and line_pair written to device buffers) and as the size query (both builds, flags and scans
alone).  Times by events around repeated calls; every call synchronises once, which is part of what a caller pays.  Beside them the host
alternative available without the call: gx_group_lines with line_key, a download of line_key, the result rows and the text, and a
Python dict keyed by (key number, second bytes) -- timed once, on the first --host-lines lines (a million by default: the loop takes
about a microsecond and a half per line).
Usage: bench_group_pairs.py [lines] [line_bytes] [--out FILE] [--append] [--cases abc] [--host-lines M]"""
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
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_pairs.txt")
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
GROUPS = {"timestamp": 0, "verb": 1, "timeTakenInMsec": 2, "path": 3}


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


def host_alternative(parts, second, max_keys):
    """gx_group_lines with line_key on the first m lines, the downloads, the dict: seconds of wall clock for each step"""
    m = min(n, host_lines)
    lkey = torch.empty(m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc, totals = g.group_lines_device(data.data_ptr(), off.data_ptr(), m, rows.data_ptr(), None, parts, line_key_ptr=lkey.data_ptr(), max_keys=max_keys, compact=2, stream=st)
    torch.cuda.synchronize()
    assert rc == N.GX_OK
    t1 = time.perf_counter()
    h_key, h_rows, h_data = lkey.cpu().numpy().view(np.uint32), rows[:m].cpu().numpy(), data[:m * lb].cpu().numpy()
    t2 = time.perf_counter()
    by_both, raw = {}, h_data.tobytes()
    b, e = 1 + 2 * GROUPS[second], 2 + 2 * GROUPS[second]
    for i, (k, r) in enumerate(zip(h_key.tolist(), h_rows.tolist())):
        if k != 0xFFFFFFFF and r[b] != 0xFF:
            pair = (k, raw[i * lb + r[b]:i * lb + r[e]])
            by_both[pair] = by_both.get(pair, 0) + 1
    t3 = time.perf_counter()
    return m, len(by_both), t1 - t0, t2 - t1, t3 - t2


def case(label, second, max_keys, units_cap, max_pairs, pair_units_cap, bound):
    parts, seconds = g.pair_parts([(name, "verb", second) for name in names])
    both = (parts, seconds)
    units = torch.empty(max(1, units_cap), dtype=torch.uint8, device="cuda")
    koff = torch.empty(max_keys + 1, dtype=torch.int32, device="cuda")
    first = torch.empty(max_keys, dtype=torch.int32, device="cuda")
    lines = torch.empty(max_keys, dtype=torch.int64, device="cuda")
    lkey = torch.empty(n, dtype=torch.int32, device="cuda")
    punits = torch.empty(max(1, pair_units_cap), dtype=torch.uint8, device="cuda")
    poff = torch.empty(max_pairs + 1, dtype=torch.int32, device="cuda")
    pkey = torch.empty(max_pairs, dtype=torch.int32, device="cuda")
    pfirst = torch.empty(max_pairs, dtype=torch.int32, device="cuda")
    plines = torch.empty(max_pairs, dtype=torch.int64, device="cuda")
    kpairs = torch.empty(max_keys, dtype=torch.int64, device="cuda")
    lpair = torch.empty(n, dtype=torch.int32, device="cuda")
    key_out = dict(key_units_ptr=units.data_ptr(), key_units_cap=units_cap, key_offsets_ptr=koff.data_ptr(), key_first_line_ptr=first.data_ptr(),
                   key_lines_ptr=lines.data_ptr(), line_key_ptr=lkey.data_ptr(), max_keys=max_keys, compact=2, stream=st)
    full = lambda: g.group_pairs_device(*batch, both, pair_units_ptr=punits.data_ptr(), pair_units_cap=pair_units_cap, pair_offsets_ptr=poff.data_ptr(),
                                        pair_key_ptr=pkey.data_ptr(), pair_first_line_ptr=pfirst.data_ptr(), pair_lines_ptr=plines.data_ptr(),
                                        key_pairs_ptr=kpairs.data_ptr(), line_pair_ptr=lpair.data_ptr(), max_pairs=max_pairs, **key_out)
    query = lambda: g.group_pairs_device(*batch, both, max_keys=max_keys, max_pairs=max_pairs, compact=2, stream=st)
    yard = lambda: g.group_lines_device(*batch, parts, **key_out)
    yard_query = lambda: g.group_lines_device(*batch, parts, max_keys=max_keys, compact=2, stream=st)
    rc, totals = full()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and totals["exact"] and totals["pairs_exact"] and totals["lines"] == totals["keyed"] == totals["paired"] == int((cat >= 0).sum()), (rc, totals)
    k, p = totals["n_keys"], totals["n_pairs"]
    assert int(plines[:p].sum()) == totals["paired"] and int(kpairs[:k].sum()) == p and int(lines[:k].sum()) == totals["lines"]
    assert bool((torch.diff(pfirst[:p].to(torch.int64)) > 0).all()) and bool((lpair.view(torch.int32) == -1).eq(lkey.view(torch.int32) == -1).all())
    if second == "verb":
        assert p == k and bool((kpairs[:k] == 1).all()) and torch.equal(lpair, lkey)
    keys_before = (lkey.clone(), lines[:k].clone())
    rc, alone = yard()
    torch.cuda.synchronize()
    assert rc == N.GX_OK and all(totals[name] == v for name, v in alone.items()) and torch.equal(lkey, keys_before[0]) and torch.equal(lines[:k], keys_before[1])
    (ms_full, mn_full), (ms_query, mn_query), (ms_yard, mn_yard), (ms_yq, mn_yq) = timed_pair([full, query, yard, yard_query])
    say("(%s) verb x %s: %d keys, %d pairs of %d units over %d lines" % (label, second, k, p, totals["pair_units"], totals["lines"]))
    say("    gx_group_pairs, every output          %8.3f ms (min %.3f)" % (ms_full, mn_full))
    say("    gx_group_pairs, size query            %8.3f ms (min %.3f)" % (ms_query, mn_query))
    say("    gx_group_lines, every output          %8.3f ms (min %.3f)" % (ms_yard, mn_yard))
    say("    gx_group_lines, size query            %8.3f ms (min %.3f)" % (ms_yq, mn_yq))
    say("    group_pairs / group_lines = %.2f (every output), %.2f (size query)%s" % (ms_full / ms_yard, ms_query / ms_yq,
                                                                                      "; the expectation: 2.00 -- %s" % ("held" if ms_full <= 2 * ms_yard else "MISSED") if bound else "; no bound"))
    m, found, s_group, s_down, s_dict = host_alternative(parts, second, max_keys)
    say("    the host alternative on the first %d lines: gx_group_lines with line_key %.1f ms, downloads %.1f ms, a Python dict of %d pairs %.1f ms: %.1f ms, %.0f ns a line"
        % (m, s_group * 1e3, s_down * 1e3, found, s_dict * 1e3, (s_group + s_down + s_dict) * 1e3, (s_group + s_down + s_dict) * 1e9 / m))
    if m == n:
        assert found == p
    return totals, ms_full, ms_query


if "a" in cases:
    case("a", "verb", 64, 1024, 64, 1024, True)
if "b" in cases:
    case("b", "timeTakenInMsec", 64, 1024, 1 << 17, 1 << 20, True)
if "c" in cases:
    totals, ms_full, ms_query = case("c", "path", 64, 1024, n, n * lb, False)
    slots = 64
    while slots < 2 * n:
        slots *= 2
    say("    pair table: %d slots x 24 B (slot word, lines, first line) + 4 B pair number = %.0f MB; per-line arrays %.0f MB" % (slots, slots * 28 / 1e6, n * 25 / 1e6))
    say("    %d claims (one compare-and-swap per pair) in the size query's %.3f ms: %.1f per us over the whole table" % (totals["n_pairs"], ms_query, totals["n_pairs"] / ms_query / 1e3))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(report) + "\n")
