#!/usr/bin/env python3
"""Developer tool: time gx_top_groups on fabricated batches of N "key value" lines (15 bytes: k + 7 digits, a blank, 6 digits), made
with torch on the device against a handle of one trivial extraction `a(.*)(.*)` -- ids 0, capture rows (0, 8, 9, 15) -- so no
extraction runs.  Next to it, in the same process and alternating round by round, the yardstick: gx_group_lines with every output on
the same batch and the same table.
  (a) six keys.  Reported: the time the new call adds over gx_group_lines, and the digits its plan selects on.
  (b) about a million distinct keys, drawn skewed; ranked by lines and by sum, the ten largest, device pointers.  The claim checked:
      gx_top_groups costs no more than gx_group_lines with every output (it emits ten keys, not a million, and adds a select over a
      million 16-byte keys).
  (c) case (b) on host arrays.  The yardstick is the loop the call replaces: gx_group_lines with host outputs, then np.lexsort on
      (key number, -value) and the first ten.
The new call's result is compared with the yardstick's before anything is timed.  Every call is timed as a caller pays for it, its own
synchronisations included.  Device cases: events around repeated calls; host cases: wall clock.
Usage: bench_top_groups.py [lines] [--out FILE] [--cases a,b,c]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "top_groups.txt")
cases = "a,b,c"
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
if "--cases" in argv:
    at = argv.index("--cases"); cases = argv[at + 1]; del argv[at:at + 2]
n = int(argv[0]) if len(argv) > 0 else 10_000_000
report = []
KEY_DIGITS, VALUE_DIGITS = 7, 6
LINE = 1 + KEY_DIGITS + 1 + VALUE_DIGITS
WANTED = 10


def say(line):
    print(line, flush=True)
    report.append(line)


g = Gorp.construct([FlattenedExtraction("r0", [["text", "a"], ["extractor", "v0", [["pattern", ".*"]]], ["extractor", "v1", [["pattern", ".*"]]]])])
st = torch.cuda.current_stream().cuda_stream
PARTS = g.group_parts([(0, 0, 1)])
say("device: %s; library %s; %d lines x %d bytes, int32 ids and dense capture rows" % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, LINE))


def fabricate(names, values):
    """the batch on the device: data, offsets, ids, capture rows"""
    data = torch.empty((n, LINE), dtype=torch.uint8, device="cuda")
    data[:, 0] = ord("k")
    data[:, 1 + KEY_DIGITS] = 0x20
    for d in range(KEY_DIGITS):
        data[:, KEY_DIGITS - d] = ((names // 10 ** d) % 10 + 48).to(torch.uint8)
    for d in range(VALUE_DIGITS):
        data[:, LINE - 1 - d] = ((values // 10 ** d) % 10 + 48).to(torch.uint8)
    off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * LINE).to(torch.int32)
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    caps = torch.tensor([0, 1 + KEY_DIGITS, 2 + KEY_DIGITS, LINE], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
    return data.reshape(-1), off, ids, caps


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


def timed_host(calls, rounds=5):
    ts = [[] for _ in calls]
    for call in calls:
        call()
    for _ in range(rounds):
        for c, call in enumerate(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ts[c].append((time.perf_counter() - t0) * 1e3)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def plan_digits(values):
    """the 8-bit digits in which two of the rank values' 128-bit keys differ (gx_top_groups.hpp: tg_plan), 15 = the top one; the values
    here are non-negative and below 2^63, so the keys' high words are all the same"""
    assert values.min() >= 0
    differ = int(np.bitwise_or.reduce(values)) ^ int(np.bitwise_and.reduce(values))
    return [d for d in range(15, -1, -1) if (differ >> (8 * d)) & 0xFF]


def device_case(label, names, values, max_keys, bys):
    data, off, ids, caps = fabricate(names, values)
    batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
    # the yardstick's buffers: every output of gx_group_lines
    rc, totals = g.group_lines_device(*batch, PARTS, max_keys=max_keys, stream=st)
    assert rc == N.GX_OK and totals["exact"], (rc, totals)
    k, units_all = totals["n_keys"], totals["key_units"]
    y_units = torch.empty(units_all, dtype=torch.uint8, device="cuda")
    y_off = torch.empty(k + 1, dtype=torch.int32, device="cuda")
    y_first = torch.empty(k, dtype=torch.int32, device="cuda")
    y_lines = torch.empty(k, dtype=torch.int64, device="cuda")
    y_stats = torch.empty((k, 8), dtype=torch.int64, device="cuda")
    y_lkey = torch.empty(n, dtype=torch.int32, device="cuda")
    # (max_keys sizes the table and must hold the keys; the per-key arrays hold exactly k)
    group = lambda: g.group_lines_device(*batch, PARTS, key_units_ptr=y_units.data_ptr(), key_units_cap=units_all, key_offsets_ptr=y_off.data_ptr(),
                                         key_first_line_ptr=y_first.data_ptr(), key_lines_ptr=y_lines.data_ptr(), key_stats_ptr=y_stats.data_ptr(),
                                         line_key_ptr=y_lkey.data_ptr(), max_keys=max_keys, stream=st)
    t_units = torch.empty(WANTED * KEY_DIGITS * 2, dtype=torch.uint8, device="cuda")
    t_off = torch.empty(WANTED + 1, dtype=torch.int32, device="cuda")
    t_num = torch.empty(WANTED, dtype=torch.int32, device="cuda")
    t_first = torch.empty(WANTED, dtype=torch.int32, device="cuda")
    t_lines = torch.empty(WANTED, dtype=torch.int64, device="cuda")
    t_stats = torch.empty((WANTED, 8), dtype=torch.int64, device="cuda")
    t_lrank = torch.empty(n, dtype=torch.int32, device="cuda")

    def top(by, line_rank=False):
        return lambda: g.top_groups_device(*batch, PARTS, WANTED, by=by, key_units_ptr=t_units.data_ptr(), key_units_cap=t_units.numel(), key_offsets_ptr=t_off.data_ptr(),
                                           key_number_ptr=t_num.data_ptr(), key_first_line_ptr=t_first.data_ptr(), key_lines_ptr=t_lines.data_ptr(),
                                           key_stats_ptr=t_stats.data_ptr(), line_rank_ptr=t_lrank.data_ptr() if line_rank else None, cap_keys=WANTED,
                                           max_keys=max_keys, stream=st)
    rc, _ = group()
    torch.cuda.synchronize()
    assert rc == N.GX_OK
    say("(%s) %d keys of %d lines, %d key units; table for max_keys = %d" % (label, k, n, units_all, max_keys))
    yard = None
    for by in bys:
        v = y_lines[:k].cpu().numpy() if by == "lines" else y_stats[:k, 6].cpu().numpy()     # (sums here fit 64 bits: sum_lo is the sum)
        order = np.lexsort((np.arange(k), -v))[:WANTED]
        rc, t = top(by)()
        torch.cuda.synchronize()
        assert rc == N.GX_OK and t["n_top"] == min(WANTED, k) and t["candidates"] == k, (rc, t)
        assert t_num[:t["n_top"]].cpu().tolist() == order.tolist() and t["last"] == int(v[order[-1]]), (by, t)
        digits = plan_digits(v)
        (ms_new, mn_new), (ms_rank, mn_rank), (ms_group, mn_group) = timed([top(by), top(by, True), group])
        yard = (ms_group, mn_group)
        say("    by %-5s  gx_top_groups, %d keys, every per-key output   %9.3f ms (min %.3f)" % (by, WANTED, ms_new, mn_new))
        say("              ... and line_rank                              %9.3f ms (min %.3f)" % (ms_rank, mn_rank))
        say("              gx_group_lines, every output (yardstick)       %9.3f ms (min %.3f)" % (ms_group, mn_group))
        say("              new / yardstick = %.3f (added: %+.3f ms); the plan selects on %d of 16 digits: %s" %
            (ms_new / ms_group, ms_new - ms_group, len(digits), digits))
        if label == "b" and ms_new > ms_group:
            say("              THE NEW CALL COSTS MORE THAN gx_group_lines WITH EVERY OUTPUT")
    return data, off, ids, caps, k, yard


def host_case(label, names, values, max_keys, bys):
    data, off, ids, caps = [t.cpu().numpy() for t in fabricate(names, values)]
    torch.cuda.synchronize()
    batch = (data.ctypes.data, off.ctypes.data, n, ids.ctypes.data, caps.ctypes.data)
    rc, totals = g.group_lines_device(*batch, PARTS, max_keys=max_keys, device_pointers=False)
    assert rc == N.GX_OK and totals["exact"], (rc, totals)
    k, units_all = totals["n_keys"], totals["key_units"]
    y_units, y_off, y_first = np.empty(units_all, np.uint8), np.empty(k + 1, np.uint32), np.empty(k, np.uint32)
    y_lines, y_stats, y_lkey = np.empty(k, np.uint64), np.empty((k, 8), np.int64), np.empty(n, np.uint32)
    t_units, t_off, t_num, t_first = np.empty(WANTED * KEY_DIGITS * 2, np.uint8), np.empty(WANTED + 1, np.uint32), np.empty(WANTED, np.uint32), np.empty(WANTED, np.uint32)
    t_lines, t_stats = np.empty(WANTED, np.uint64), np.empty((WANTED, 8), np.int64)
    say("(%s) %d keys of %d lines on host arrays: the batch is staged by both sides" % (label, k, n))
    for by in bys:
        def loop():
            rc, _ = g.group_lines_device(*batch, PARTS, key_units_ptr=y_units.ctypes.data, key_units_cap=units_all, key_offsets_ptr=y_off.ctypes.data,
                                         key_first_line_ptr=y_first.ctypes.data, key_lines_ptr=y_lines.ctypes.data, key_stats_ptr=y_stats.ctypes.data,
                                         line_key_ptr=y_lkey.ctypes.data, max_keys=max_keys, device_pointers=False)
            assert rc == N.GX_OK
            v = y_lines.astype(np.int64) if by == "lines" else y_stats[:, 6]
            order = np.lexsort((np.arange(k), -v))[:WANTED]
            return order, v[order]

        def new():
            rc, t = g.top_groups_device(*batch, PARTS, WANTED, by=by, key_units_ptr=t_units.ctypes.data, key_units_cap=t_units.size, key_offsets_ptr=t_off.ctypes.data,
                                        key_number_ptr=t_num.ctypes.data, key_first_line_ptr=t_first.ctypes.data, key_lines_ptr=t_lines.ctypes.data,
                                        key_stats_ptr=t_stats.ctypes.data, cap_keys=WANTED, max_keys=max_keys, device_pointers=False)
            assert rc == N.GX_OK
            return t
        order, v = loop()
        t = new()
        assert t_num.tolist() == order.tolist() and t["last"] == int(v[-1])
        (ms_new, mn_new), (ms_loop, mn_loop) = timed_host([new, loop], rounds=3)
        say("    by %-5s  gx_top_groups on host arrays                           %9.3f ms (min %.3f)" % (by, ms_new, mn_new))
        say("              gx_group_lines on host arrays + np.lexsort (the loop)  %9.3f ms (min %.3f): %.2f x" % (ms_loop, mn_loop, ms_loop / ms_new))


gen = torch.Generator(device="cuda")
gen.manual_seed(2)
values = torch.randint(0, 10 ** VALUE_DIGITS, (n,), device="cuda", generator=gen)
for c in cases.split(","):
    if c == "a":
        device_case("a", torch.randint(0, 6, (n,), device="cuda", generator=gen), values, 64, ["lines", "sum"])
    elif c in ("b", "c"):
        spread = n // 9                                   # drawn skewed: name = spread * u^3 -- the head holds most lines, the tail one or two each
        names = torch.clamp((spread * torch.rand(n, device="cuda", generator=gen) ** 3).to(torch.int64), max=min(spread, 10 ** KEY_DIGITS) - 1)
        if c == "b":
            device_case("b", names, values, n // 8, ["lines", "sum"])
        else:
            host_case("c", names, values, n // 8, ["lines", "sum"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
