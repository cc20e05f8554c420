"""bench.py --dump-outputs on the HIP kernels: one small run (ResNet-18, 32 images of 64x64), default path."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_of_the_default_hip_path(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "IMAGENT_DETERMINISTIC"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--arch", "resnet18",
                        "--batch-size", "32", "--image-size", "64", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "d")], cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    # the dumping run is the plain run: default (non-deterministic) HIP path, no instrumented steps
    assert out["config"]["kernels"] == "hip" and out["config"]["deterministic"] is False
    assert out["config"]["comm_overlap"] is None and out["steps"] == 3 and out["ms_per_step"] > 0
    a = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    # the whole gradient / momentum only with --deterministic 1 (they do not repeat on the default path)
    assert set(a) == {"parameters", "gradient_fc_bias", "bn_running_mean", "bn_running_var", "metrics"}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    # the last step alone: 32 images, a loss near ln(1000) at random init
    assert a["metrics"][3] == 32 and 3.0 < a["metrics"][0] / 32 < 12.0
    # d loss / d fc.bias = mean over the batch of (softmax - onehot): its 1000 entries sum to zero. The gradient of
    # the logits is bf16 (2^-9 relative per entry): 32 label entries of ~1/32 and 1000 softmax entries of ~1e-3
    # give at most 32 * 6e-5 + 1000 * 2e-6 = 4e-3, doubled for the fp32 sums
    assert a["gradient_fc_bias"].shape == (1000,) and abs(a["gradient_fc_bias"].sum()) <= 8e-3
    assert np.abs(a["gradient_fc_bias"]).max() > 1e-3
    # one step from the seeded initial state (running mean 0, running var 1, momentum 0.1): var = 0.9 + 0.1 * batch
    # var >= 0.9; four steps without the rewind would leave 0.9^4 = 0.66 of the initial 1
    assert a["bn_running_var"].min() >= 0.9 - 1e-3 and np.abs(a["bn_running_mean"]).max() > 0
