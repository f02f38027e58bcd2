"""bench.py's command line: a plain run times the headline steps and nothing else; ``--dump-outputs DIR`` writes what
the last timed step handed back; ``--full`` adds the secondary measurements (tests/test_gpu_data_parallel.py runs it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _plain_run(steps, warmup, out_dir):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--frames", "6",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    names = sorted(p.name for p in out_dir.iterdir())
    assert names == ["adam_exp_avg.npy", "adam_exp_avg_sq.npy", "grads.npy", "loss.npy", "params.npy"], names
    return json.loads(lines[0]), {n[:-4]: np.load(out_dir / n) for n in names}


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_only_and_dumps_the_last_step(tmp_path):
    steps, warmup = 3, 1
    out, arrays = _plain_run(steps, warmup, tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == steps and out["warmup"] == warmup and out["unit"] == "rays/s" and out["dtype"] == "bf16"
    assert abs(out["value"] - 4096 / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]
    # nothing that only --full measures
    for key in ("kernels_in_step", "value_fp8_images", "kernels", "rooflines", "render_fps", "cpu_baseline", "instant", "part4"):
        assert key not in out, key
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays["loss"]) == pytest.approx(out["final_loss"], rel=1e-6)
    assert arrays["params"].shape == arrays["grads"].shape == arrays["adam_exp_avg"].shape
    assert float(np.abs(arrays["grads"]).max()) > 0.0 and float(arrays["adam_exp_avg_sq"].max()) > 0.0
    # the same arguments give the same inputs, and the weight gradients are summed in a fixed order: the training state
    # after the last timed step is reproduced bit for bit (the loss sum may take a float atomic: tolerance)
    _, again = _plain_run(steps, warmup, tmp_path / "b")
    for name in ("params", "grads", "adam_exp_avg", "adam_exp_avg_sq"):
        assert np.array_equal(arrays[name], again[name]), name
    assert float(again["loss"]) == pytest.approx(float(arrays["loss"]), rel=1e-6)
    # ... and it is the state after the LAST timed step: one step more moves the weights and both moments
    _, longer = _plain_run(steps + 1, warmup, tmp_path / "c")
    for name in ("params", "adam_exp_avg", "adam_exp_avg_sq"):
        assert not np.array_equal(arrays[name], longer[name]), name
