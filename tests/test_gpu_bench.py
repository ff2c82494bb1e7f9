"""-m gpu: what a plain `bench.py` run prints and what `--full` adds to it, at a small size (64 trajectories x 5001 samples)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--batch", "64", "--nt", "5001", "--steps", "2", "--warmup", "1"]


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(gpu):
    """A plain run prints the headline and its `config` / `roofline` and nothing that takes work of its own; `--full` computes the same
    headline solve and adds the CPU baseline, whose C oracle leg re-checks the GPU's trajectories."""
    plain = _bench()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["unit"] == "trajectories/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["value"] > 0 and plain["config"]["trajectories_ok"] == 64
    assert "cpu_baseline" not in plain and "cpu_baseline_python" not in plain and "traffic_stale" not in plain["roofline"]
    full = _bench("--full", "--no-python-baseline", "--cpu-sample", "16")
    for k in ("loss", "mean_nfe", "max_nfe", "mean_accepted", "mean_rejected", "trajectories_ok", "kernel"):
        assert full["config"][k] == plain["config"][k], k
    cb = full["cpu_baseline"]
    assert cb["value"] > 0 and cb["rel_l2_gpu_vs_oracle"] <= 1e-12, cb
    assert "cpu_baseline_python" not in full
