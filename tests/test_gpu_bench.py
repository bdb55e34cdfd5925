"""bench.py on one GPU: a plain run times exactly --steps steps and carries the headline only (the legs beyond it need
--full); `--dump-outputs DIR` writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_requested_steps_and_dumps_the_last_one(tmp_path):
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "64", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == r["steps_requested"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert (r["unit"], r["higher_is_better"], r["dtype"]) == ("windows/s", True, "f32") and r["value"] > 0
    assert not {"roofline", "fp32_mfma", "infer_windows_per_s", "leads2", "conv_stage_roofline", "cpu_baseline"} & set(r)
    assert sorted(os.listdir(d)) == ["loss.npy", "params.npy", "pred.npy", "rmse.npy", "snr.npy"]
    pred, loss, snr = np.load(d / "pred.npy"), np.load(d / "loss.npy"), np.load(d / "snr.npy")
    assert pred.shape == (64, 1, 512) and pred.dtype == np.float32 and np.isfinite(pred).all()
    assert snr.shape == (64,) and np.isfinite(snr).all()
    assert loss.dtype == np.float64 and abs(loss[0] - r["final_loss"]) <= 1e-6 + 1e-6 * abs(r["final_loss"])
    params = np.load(d / "params.npy")
    assert params.dtype == np.float32 and params.size > 1000 and np.isfinite(params).all()
