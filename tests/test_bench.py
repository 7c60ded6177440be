"""bench.py's command line: what a plain run prints, and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _fake_fetch(idx):
    return (idx % 7 - 2).astype(np.int32), ((idx[:, None] * 3 + np.arange(6)[None, :]) % 300 - 1).astype(np.int32)


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in ("match_id", "captures", "line_index")}


def test_write_outputs_small_batch_is_written_whole(tmp_path):
    n = 1000
    bench.write_outputs(str(tmp_path / "out"), n, 6, _fake_fetch)
    got = _load(str(tmp_path / "out"))
    assert got["match_id"].dtype == np.float32 and got["captures"].dtype == np.float32 and got["line_index"].dtype == np.float64
    assert got["line_index"].tolist() == list(range(n))
    want_m, want_c = _fake_fetch(np.arange(n))
    assert np.array_equal(got["match_id"], want_m) and np.array_equal(got["captures"], want_c)


def test_write_outputs_large_batch_is_a_fixed_sample_under_64_mb(tmp_path):
    n = 10_000_000
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.write_outputs(a, n, 6, _fake_fetch)
    bench.write_outputs(b, n, 6, _fake_fetch)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert sorted(os.listdir(a)) == ["captures.npy", "line_index.npy", "match_id.npy"] and total <= 64 << 20
    ga, gb = _load(a), _load(b)
    idx = ga["line_index"].astype(np.int64)
    k = len(idx)
    assert 0 < k < n and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert ga["captures"].shape == (k, 6) and ga["match_id"].shape == (k,)
    want_m, want_c = _fake_fetch(idx)
    assert np.array_equal(ga["match_id"], want_m) and np.array_equal(ga["captures"], want_c)
    for name in ga:
        assert np.array_equal(ga[name], gb[name]), name


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_what_it_computed(tmp_path):
    """A plain run prints the headline line without the --full extras, and --dump-outputs holds the timed path's results:
    the same ids and capture offsets as the oracle's for the same seeded lines."""
    import torch
    from gorp_amd import workloads as W
    from oracle import oracle as O
    lines = 200_000
    out_dir = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--lines", str(lines), "--steps", "4", "--warmup", "2",
                        "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out_lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(out_lines) == 1, r.stdout[-2000:]
    out = json.loads(out_lines[0])
    for key in HEADLINE_KEYS:
        assert key in out, key
    assert out["steps"] == 4 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "lines/s"
    assert out["config"]["lines_per_gpu"] == lines
    for key in ("also", "cpu_baseline", "formats", "one_line_latency_us"):
        assert key not in out, key
    got = _load(out_dir)
    idx = got["line_index"].astype(np.int64)
    assert idx.tolist() == list(range(lines))    # (a batch this small fits whole)
    definition = W.readme3_definition()
    data, offsets, _ = W.readme3_lines(lines, seed=2, device="cuda")   # bench.py's config 2 shard of rank 0
    built = [e.build() for e in definition]
    omid, ocaps = O.OracleGorp([b[0] for b in built], [b[1] for b in built]).extract_batch(
        data.cpu().numpy(), offsets.cpu().numpy().astype(np.uint32), nthreads=4)
    del data, offsets
    torch.cuda.empty_cache()
    assert np.array_equal(got["match_id"], omid.astype(np.float32))
    assert np.array_equal(got["captures"], ocaps.astype(np.float32))
