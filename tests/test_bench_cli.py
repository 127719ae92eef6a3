"""bench.py's launch rules on CPU (no GPU call is reached): --gpus N is
honoured or refused, never silently run as one rank."""
from __future__ import annotations

import os
import subprocess
import sys

from conftest import ROOT


def _run(args, **env_over):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_DIST_BACKEND"):
        env.pop(k, None)
    env.update(env_over)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_world_size_and_gpus_flag_must_agree():
    r = _run(["--gpus", "2", "--steps", "1"], WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "disagree" in r.stderr, r.stderr[-2000:]
    assert "{" not in r.stdout


def test_gpus_flag_with_rccl_needs_that_many_gpus():
    """Here (no GPU visible) --gpus 2 over RCCL must fail fast, before any
    rank starts, instead of printing an n_gpus: 1 line."""
    import torch

    if torch.cuda.device_count() >= 2:  # (a multi-GPU host would run it for real)
        return
    r = _run(["--gpus", "2", "--steps", "1"])
    assert r.returncode == 2 and "visible GPUs" in r.stderr, r.stderr[-2000:]
    assert "{" not in r.stdout


def test_gpus_flag_must_be_positive():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0 and "--gpus" in r.stderr


def test_extra_measurements_need_full():
    """--two-streams / --host-sweep belong to --full: asked for without it
    they are refused, not silently dropped."""
    for flag in ("--two-streams", "--host-sweep"):
        r = _run(["--gpus", "1", "--steps", "1", flag])
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
        assert "{" not in r.stdout


def test_dump_outputs_is_exact_and_samples_large_arrays_the_same_way(tmp_path):
    """--dump-outputs: 32-bit checksums survive float64 exactly; an array past
    the cap is cut to a fixed sample (the same indices in every run); rank
    r > 0 writes a file of its own."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    small = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF], np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), 0, small.view(np.int32))  # (the device arrays are int32 views)
    got = np.load(tmp_path / "a" / "checksums.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), small)
    big = (np.arange(bench.DUMP_MAX_VALUES + 12345, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    bench.dump_outputs(str(tmp_path / "b"), 0, big)
    bench.dump_outputs(str(tmp_path / "c"), 1, big)
    b = np.load(tmp_path / "b" / "checksums.npy")
    c = np.load(tmp_path / "c" / "checksums_rank1.npy")
    assert b.shape == (bench.DUMP_MAX_VALUES,) and b.nbytes <= 64 << 20 and np.array_equal(b, c)
    assert np.isin(b.astype(np.uint32), big).all() and len(np.unique(b)) > bench.DUMP_MAX_VALUES // 2


def test_sub_run_error_is_reported_in_its_sub_object():
    """A sub-run that raises is recorded in its sub-object and the runs after
    it are skipped; the main line is still printed once (publish)."""
    sys.path.insert(0, ROOT)
    import bench

    line = {"metric": "m", "config4": None, "strong_scaling": None}
    wd = bench.SubRunWatchdog(60.0, line)

    def boom():
        raise RuntimeError("rccl init failed")

    bench.line_set(line, "config4", wd.run("config4", boom))
    assert wd.failed and line["config4"] == {"error": "RuntimeError: rccl init failed"}
    assert wd.run("ok", lambda: {"x": 1}) == {"x": 1}
    wd.cancel()


_WATCHDOG_SCRIPT = r"""
import sys, time
sys.path.insert(0, %r)
import bench
line = {"metric": "m", "value": 1.0, "config4": {"kernel_step_us": 24.0}, "strong_scaling": None}
wd = bench.SubRunWatchdog(0.5, line)
wd.start()
wd.run("strong_scaling", time.sleep, 30)
print("not reached")
"""


def test_sub_run_watchdog_prints_the_main_line_and_exits():
    """A hung sub-run (here a sleep standing in for a collective no peer
    joins): past the bound the main line is printed once, with the finished
    sub-object kept and the hung one marked, and the process exits 0."""
    import json

    r = subprocess.run([sys.executable, "-c", _WATCHDOG_SCRIPT % ROOT], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "not reached" not in r.stdout
    d = json.loads(lines[0])
    assert d["config4"] == {"kernel_step_us": 24.0}
    assert "timed out" in d["strong_scaling"]["error"] and "strong_scaling" in d["strong_scaling"]["error"]
    assert "watchdog fired" in r.stderr
