#!/usr/bin/env python3
"""Developer tool: what gx_batch_opts.utf8 costs.  Config 2 (README definition, N x 200-byte lines on the device, u8 result rows)
with 0 %, 1 %, 10 % and 100 % of the lines carrying one 3-byte character in their path; per share, in ms per call: utf8 = 1 with
the flag sweep, utf8 = 1 with the line flags supplied, utf8 = 2 -- each next to the same batch without utf8 on the same device in
the same run (the floor: bytes read as Latin-1).  For 100 %: the utf16 batch path on the units gx_utf8_to_utf16 makes of the batch,
and gx_utf8_to_utf16 alone next to a copy_ of as many bytes as it reads and writes -- and the same two once more with a two-byte
character below U+0100 in every line, which the utf16 batch path narrows instead of walking the line again.  For 0 % and 1 %:
gx_text_to_jsonl on the same lines with utf8 next to the same text as bytes with pass-through.  Times by events around repeated
synchronous calls (a utf8 batch reads two numbers on the host, which is part of what a caller pays); warm-up as DESIGN.md section 6
describes.
With a list of shares (e.g. 0.01 or 0,1) only those are run: one share per rocprofv3 --kernel-trace --stats run gives that
share's per-kernel times ("batch" behind the shares leaves the 100 % baselines out of such a run).
Usage: bench_utf8.py [lines] [line_bytes] [shares] [batch]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gorp_amd import _native as N
if os.environ.get("GX_BENCH_LIB"):   # another build of the library (A/B runs)
    N.LIB_PATH = os.path.abspath(os.environ["GX_BENCH_LIB"])
from gorp_amd import workloads as W
from gorp_amd.gorp import Gorp, utf8_to_utf16_device

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
lb = int(sys.argv[2]) if len(sys.argv) > 2 else W.LINE_BYTES
shares = [float(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0.0, 0.01, 0.10, 1.0]
g = Gorp.construct(W.readme3_definition())
data, off, cat = W.readme3_lines(n, seed=2, device="cuda", line_bytes=lb)
width = 1 + 2 * g.max_groups
rows = torch.empty((n, width), dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
ZHONG = torch.tensor([0xE4, 0xB8, 0xAD], dtype=torch.uint8, device="cuda")
E_ACUTE = torch.tensor([0xC3, 0xA9], dtype=torch.uint8, device="cuda")


def timed(call, rounds=5):
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    once = time.perf_counter() - t0
    reps = max(1, min(10, int(0.1 / max(once, 1e-4))))
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


def extract(text, utf8=0, flags=None):
    g.extract_batch_device(text.data_ptr(), off.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb, max_line_bytes=lb, compact=2,
                           utf8=utf8, utf8_line_flags_ptr=flags.data_ptr() if flags is not None else None)


def baselines(text, label, ms_utf8_2, ids_floor):
    """100 %: gx_utf8_to_utf16 alone beside a copy_ of as many bytes, and the utf16 batch path on its units."""
    total = utf8_to_utf16_device(text.data_ptr(), off.data_ptr(), n, None, 0, None, stream=st)
    u = torch.empty(total, dtype=torch.int16, device="cuda")
    uoff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ms_t = timed(lambda: utf8_to_utf16_device(text.data_ptr(), off.data_ptr(), n, u.data_ptr(), total, uoff.data_ptr(), stream=st))
    moved = text.numel() + 4 * (n + 1) + 2 * total + 4 * (n + 1)
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    ms_c = timed(lambda: dst.copy_(src))   # (a copy of b bytes reads b and writes b: half of what the call moves each way)
    ms_16 = timed(lambda: g.extract_batch_device(u.data_ptr(), uoff.data_ptr(), n, None, rows.data_ptr(), stream=st, line_bytes_hint=lb,
                                                 max_line_bytes=lb, compact=2, utf16=True))
    assert torch.equal(rows[:, 0], ids_floor)
    print("100 %% %s: gx_utf8_to_utf16 alone %.3f ms (min %.3f): %d units, %.3f GB read + written; copy_ moving as many bytes %.3f ms (x%.1f)"
          % (label, ms_t[0], ms_t[1], total, moved / 1e9, ms_c[0], ms_t[0] / ms_c[0]))
    print("100 %% %s: utf16 batch path on those units %.3f ms (min %.3f); transcode + utf16 batch %.3f ms; utf8=2 %.3f ms"
          % (label, ms_16[0], ms_16[1], ms_t[0] + ms_16[0], ms_utf8_2))


def jsonl(text, share):
    """gx_text_to_jsonl on the same lines, '\\n' behind each: as bytes with pass-through, and with utf8 (line flags from the split
    pass in the escape bits' place, so the sizes pass reads the text once more)."""
    raw = torch.cat([text.view(n, lb), torch.full((n, 1), 10, dtype=torch.uint8, device="cuda")], dim=1).reshape(-1)
    size = g.text_to_jsonl_device(raw.data_ptr(), raw.numel(), None, 0, id_as="id", utf8=True, stream=st)[0]
    out = torch.empty(size + 64, dtype=torch.uint8, device="cuda")
    ms = [timed(lambda: g.text_to_jsonl_device(raw.data_ptr(), raw.numel(), out.data_ptr(), size + 64, id_as="id", stream=st, **kw))[0]
          for kw in (dict(utf8_passthrough=True), dict(utf8=True))]
    print("%g %%: gx_text_to_jsonl, %.3f GB of JSON text: bytes with pass-through %.3f ms, utf8 %.3f ms" % (100 * share, size / 1e9, ms[0], ms[1]))


print("device: %s; %d lines x %d bytes, u8 result rows of %d bytes" % (torch.cuda.get_device_name(0), n, lb, width))
print("%-6s %22s %22s %22s %22s   %s" % ("share", "without utf8 (floor)", "utf8=1, sweep", "utf8=1, flags given", "utf8=2, sweep", "lines walked again, units"))
for share in shares:
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    marked = torch.rand(n, device="cuda", generator=gen) < share
    text = data.clone()
    text.view(n, lb)[marked, 100:103] = ZHONG   # (inside the path: the outcome stays, the last capture holds the character)
    flags = marked.to(torch.uint8)
    cells = [timed(lambda: extract(text))]
    ids_floor = rows[:, 0].clone()
    cells.append(timed(lambda: extract(text, 1)))
    walked, units = g.stat(33), g.stat(34)
    assert walked == int(marked.sum()) and torch.equal(rows[:, 0], ids_floor)   # (\S takes the character either way)
    cells.append(timed(lambda: extract(text, 1, flags)))
    assert g.stat(33) == walked
    cells.append(timed(lambda: extract(text, 2)))
    print("%-6s " % ("%g %%" % (100 * share)) + " ".join("%10.3f (min %7.3f)" % c for c in cells) + "   %d, %d" % (walked, units))
    if share <= 0.01 and sys.argv[4:5] != ["batch"]:
        jsonl(text, share)
    if share == 1.0 and sys.argv[4:5] != ["batch"]:
        baselines(text, "U+4E2D", cells[3][0], ids_floor)
        # a character below U+0100 in every line: the utf16 batch path narrows such units and walks no line again
        text.view(n, lb)[:, 100:102] = E_ACUTE
        text.view(n, lb)[:, 102] = 0x61
        baselines(text, "U+00E9", timed(lambda: extract(text, 2))[0], ids_floor)
    del text, flags, marked
