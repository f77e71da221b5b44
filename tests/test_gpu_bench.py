"""bench.py on the GPU, every leg of its --full run switched on (short): the line must come out whole. (Round 6: the full run
crashed on a value read after the step's tensors had been released for the secondary configurations, while every flag
combination the tests and the profiling scripts used went through.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_default_legs_produce_the_whole_line():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "5", "--warmup", "2", "--psnr-steps", "20",
                          "--nerf-steps", "10", "--cpu-samples", "4096", "--cpu-budget-s", "1"], env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["metric"].startswith("hash-grid samples/sec") and rec["n_gpus"] == 1 and rec["steps"] == 5
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["dtype"] == "f32" and rec["vs_baseline"] is None
    roof = rec["roofline"]
    assert roof["bound"] == "hbm" and 0 < roof["frac"] < 1 and set(roof["operators"]) == {"forward", "backward"}
    assert rec["cpu_baseline"]["kind"] == "port" and rec["cpu_baseline"]["value"] > 0
    assert rec["config"]["plan_bytes"] > 0 and rec["config"]["backward_workspace_bytes"] > 0
    assert len(rec["other_configs_1gpu"]) >= 8 and "psnr" in rec and "psnr_nerf" in rec


@pytest.mark.gpu
def test_bench_plain_run_times_only_its_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full): the headline fields, the requested number of timed steps, none of the secondary legs, and
    --dump-outputs writes the last step's features (a fixed sample of rows) and codebook gradient (whole) in float32."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["metric"].startswith("hash-grid samples/sec") and rec["unit"] == "samples/s" and rec["higher_is_better"] is True
    assert rec["steps"] == 7 and rec["dtype"] == "f32" and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - rec["config"]["samples_per_gpu"] / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert rec["config"]["full"] is False and 0 < rec["roofline"]["frac"] < 1
    assert rec["psnr"] is None and rec["psnr_nerf"] is None and rec["other_configs_1gpu"] is None
    assert rec["cpu_baseline"] is None and rec["roofline"]["bound_model"] is None
    feats, grad = np.load(tmp_path / "features.npy"), np.load(tmp_path / "grad_codebook.npy")
    assert feats.dtype == np.float32 and feats.shape == (65536, 32) and np.isfinite(feats).all()
    assert grad.dtype == np.float32 and grad.shape == (rec["config"]["table_rows"], 2) and np.isfinite(grad).all()
    assert np.abs(grad).max() > 0 and feats.nbytes + grad.nbytes <= 64e6
