"""bench.py's command line on the GPU: a plain run times the steps and prints the headline line without the secondary
measurements (those need --full); --dump-outputs writes what the last timed step computed, from the same inputs on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "classifier_loss", "classifier_acc", "g_loss", "l_loss", "img_g", "img_l", "txt_g", "txt_l", "probs", "idx", "cap_lens",
         "grads")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "tiny", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in os.listdir(d):
        assert f.endswith(".npy"), f
        out[f[:-len(".npy")].removesuffix("_sample")] = np.load(os.path.join(d, f))
    return out


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["global_batch"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None and "module_path" not in d and "cpu_baseline" not in d
    a = _load(tmp_path / "a")
    assert set(a) == set(NAMES), sorted(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), k
    assert abs(float(a["loss"]) - d["config"]["loss"]) <= 1e-6 * max(1.0, abs(d["config"]["loss"]))
    B = d["config"]["per_gpu_batch"]
    assert a["img_g"].shape[0] == B and a["probs"].shape[0] == B and a["cap_lens"].shape == (B,)
    # a second run computes the same: every step starts from the same state, so the outputs agree to rounding (the losses and the
    # weight gradients sum in fp32 atomics) and the expert choices exactly
    _bench("--dump-outputs", str(tmp_path / "b"))
    b = _load(tmp_path / "b")
    assert set(b) == set(a) and all(b[k].shape == a[k].shape for k in a)
    assert np.array_equal(a["cap_lens"], b["cap_lens"]) and np.array_equal(a["idx"], b["idx"])
    for k in a:
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        assert np.abs(x - y).max() <= 1e-4 * max(np.abs(x).max(), 1e-6), (k, np.abs(x - y).max(), np.abs(x).max())
