#!/usr/bin/env python3
"""Developer tool: time gx_lookup_lines on N fabricated lines on the device -- a line is its key in 6 digits, a number in 10 digits and a
byte of filler, over a handle of one trivial extraction with dense int32 capture rows made here (the tests' scheme) -- with about N / 100
keys in no order at all.  Two dictionaries, both on the device: the batch's own keys as gx_group_lines left them (every line hits; the
round trip that shares key numbers between batches), and a blocklist of 1 000 of them (1 % of the lines hit).  In the same process, taking
turns round by round:
  gx_lookup_lines against the keys: the size query; line_entry, entry_lines and entry_stats written; the same with KEEP_OTHERS (nothing kept);
  gx_lookup_lines against the blocklist: the size query; KEEP_HITS and KEEP_OTHERS with the kept batch written;
  gx_group_lines on the same batch, size query and with line_key, key_lines and key_stats: the yardstick, since it hashes the same keys and
      inserts where the lookup only finds;
  the host path, for scale: the download of line_key and of the keys, and a Python set built from the blocklist probed per key.
No ratio is fixed in advance.  Times by events around repeated calls after a warm-up, median and minimum over the rounds; every call
synchronises as often as it does for any caller, which is part of what a caller pays.
Usage: bench_lookup.py [lines] [--out FILE]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd.gorp import FlattenedExtraction, Gorp

argv = list(sys.argv[1:])
out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lookup_lines.txt")
if "--out" in argv:
    at = argv.index("--out"); out_path = argv[at + 1]; del argv[at:at + 2]
n = int(argv[0]) if argv else 10_000_000
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


KD, TD = 6, 10
W = KD + TD + 1
n_keys = max(1, n // 100)
g = Gorp.construct([FlattenedExtraction("r0", [["text", "a"]] + [["extractor", "v%d" % q, [["pattern", ".*"]]] for q in range(2)])])
gen = torch.Generator(device="cuda").manual_seed(2)
key = torch.randint(0, n_keys, (n,), generator=gen, device="cuda", dtype=torch.int64)
t = torch.randint(0, 10 ** 9, (n,), generator=gen, device="cuda", dtype=torch.int64)
data = torch.full((n, W), 0x2E, dtype=torch.uint8, device="cuda")
q = key.clone()
for d in range(KD - 1, -1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
q = t.clone()
for d in range(KD + TD - 1, KD - 1, -1):
    data[:, d] = (48 + q % 10).to(torch.uint8); q //= 10
off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * W).to(torch.int32)
ids = torch.zeros(n, dtype=torch.int32, device="cuda")
caps = torch.tensor([0, KD, KD, KD + TD], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
st = torch.cuda.current_stream().cuda_stream
torch.cuda.synchronize()
batch = (data.data_ptr(), off.data_ptr(), n, ids.data_ptr(), caps.data_ptr())
parts = g.group_parts([(0, 0, 1)])
mk = 2 * n_keys
say("device: %s; library %s; %d lines x %d bytes, dense int32 rows; %d keys" % (torch.cuda.get_device_name(0), os.path.basename(N.LIB_PATH), n, W, n_keys))
i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
u8 = lambda count: torch.empty(count, dtype=torch.uint8, device="cuda")
key_units, key_off, key_lines, key_stats, line_key = u8(mk * KD), i32(mk + 1), i64(mk), i64(mk * 8), i32(n)
group_outs = dict(key_units_ptr=key_units.data_ptr(), key_units_cap=mk * KD, key_offsets_ptr=key_off.data_ptr(), key_lines_ptr=key_lines.data_ptr(),
                  key_stats_ptr=key_stats.data_ptr(), line_key_ptr=line_key.data_ptr(), max_keys=mk)
rc, gt = g.group_lines_device(*batch, parts, stream=st, **group_outs)
torch.cuda.synchronize()
assert rc == N.GX_OK and gt["exact"], (rc, gt)
k = gt["n_keys"]
# the blocklist: every 100th key or so, as a CSR of its own on the device
m_block = min(1000, k)
pick = torch.arange(m_block, device="cuda") * (k // m_block)
block_units = key_units[:k * KD].view(k, KD)[pick].contiguous().view(-1)
block_off = (torch.arange(m_block + 1, dtype=torch.int64, device="cuda") * KD).to(torch.int32)
line_entry, e_same, e_lines, e_stats = i32(n), i32(mk), i64(mk), i64(mk * 8)
o_index, o_data, o_off, o_ids, o_caps = i32(n), u8(n * W), i32(n + 1), i32(n), i32(n * 4)
entry_outs = dict(line_entry_ptr=line_entry.data_ptr(), entry_same_ptr=e_same.data_ptr(), entry_lines_ptr=e_lines.data_ptr(), entry_stats_ptr=e_stats.data_ptr())
kept_outs = dict(out_index_ptr=o_index.data_ptr(), out_data_ptr=o_data.data_ptr(), out_offsets_ptr=o_off.data_ptr(), out_ids_ptr=o_ids.data_ptr(),
                 out_caps_ptr=o_caps.data_ptr(), cap_lines=n, out_bytes_cap=n * W)
own = (key_units.data_ptr(), key_off.data_ptr(), k)
block = (block_units.data_ptr(), block_off.data_ptr(), m_block)
look = lambda d, **kw: g.lookup_lines_device(*batch, parts, *d, stream=st, **kw)

rc, lt = look(own, **entry_outs)
torch.cuda.synchronize()
assert rc == N.GX_OK and lt["misses"] == 0 and lt["hits"] == n and lt["distinct_entries"] == lt["hit_entries"] == k, lt
assert torch.equal(line_entry, line_key) and torch.equal(e_lines[:k], key_lines[:k]) and torch.equal(e_stats[:k * 8], key_stats[:k * 8])
rc, bt = look(block, keep="hits", **entry_outs, **kept_outs)
torch.cuda.synchronize()
assert rc == N.GX_OK and bt["hit_entries"] == m_block and bt["lines_out"] == bt["hits"], bt
say("%d keys; the blocklist of %d entries is hit by %d lines (%d units kept)" % (k, m_block, bt["hits"], bt["units_out"]))


def timed(calls, reps=3, rounds=7):
    """median and minimum ms per call of every call in `calls`, the calls taking turns round by round"""
    t_spin = time.perf_counter() + 0.15   # (the device's clocks need unbroken load before they are up)
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
    return [(sorted(x)[len(x) // 2], min(x)) for x in ts]


calls = [lambda: look(own), lambda: look(own, **entry_outs), lambda: look(own, keep="others", **entry_outs, **kept_outs),
         lambda: look(block), lambda: look(block, keep="hits", **entry_outs, **kept_outs), lambda: look(block, keep="others", **entry_outs, **kept_outs),
         lambda: g.group_lines_device(*batch, parts, max_keys=mk, stream=st), lambda: g.group_lines_device(*batch, parts, stream=st, **group_outs)]
labels = ["gx_lookup_lines, %d entries (all hit), size query" % k, "... line_entry and the per-entry outputs", "... and KEEP_OTHERS (nothing kept)",
          "gx_lookup_lines, %d entries (1 %% hit), size query" % m_block, "... KEEP_HITS, every output", "... KEEP_OTHERS, every output (99 % of the batch copied)",
          "gx_group_lines, size query (the yardstick)", "gx_group_lines, every output"]
res = timed(calls)
for label, (med, mn) in zip(labels, res):
    say("    %-62s %9.3f ms (min %.3f)" % (label, med, mn))

t0 = time.perf_counter()
lk = line_key.cpu().numpy()
ku = key_units[:k * KD].cpu().numpy().reshape(k, KD)
t1 = time.perf_counter()
wanted = set(bytes(r) for r in block_units.cpu().numpy().reshape(m_block, KD))
hit_key = np.fromiter((bytes(r) in wanted for r in ku), bool, k)
kept = np.flatnonzero(hit_key[lk.view(np.uint32)])
t2 = time.perf_counter()
assert len(kept) == bt["hits"]
say("    the host path, for scale: download of line_key and the keys %.1f ms; a Python set probed per key and the selection by numpy %.1f ms"
    % ((t1 - t0) * 1e3, (t2 - t1) * 1e3))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(report) + "\n")
