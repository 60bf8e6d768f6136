"""GPU: bench.py's one-line JSON contract (the driver parses it): a short plain run with the small ViT in a child
process (the bench initialises its own HIP context), the legs a plain run leaves to --full, and --dump-outputs:
the files of the last timed step's outputs and their reproduction by a second run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("clip_lift", "sustained", "multi_frame_batches", "with_h2d", "value_with_h2d", "lift_config4",
             "lift_config4_lm", "config5", "parity_3d_mm")
N_CROPS, N_JOINTS = 32, 17   # 8 views x 4 individuals per step; COCO-style joints


def _run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    return _run(d), d


def test_bench_prints_one_contract_line(plain_run):
    r, _ = plain_run
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "bf16"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is individuals x frames / s of the timed steps
    per_step = d["value"] * d["ms_per_step"] * 1e-3
    assert abs(per_step - round(per_step)) < 0.05 * per_step
    assert "workload" in d["config"]
    rl = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rl, k
    assert rl["bound"] in ("hbm", "mfma") and rl["peak"] > 0
    assert abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-3


def test_plain_run_times_the_steps_and_leaves_the_other_legs_to_full(plain_run):
    r, _ = plain_run
    d = json.loads(r.stdout.strip())
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["cpu_baseline"] is None
    # --steps sets the number of timed steps: the rank's own steps fit in the timed region, which logged 3 steps
    assert 0 < d["ranks"][0]["steps_ms"] <= d["ms_per_step"] * 3 * (1 + 1e-3)
    assert d["gather_bytes_per_rank"] == 3 * N_CROPS * N_JOINTS * 3 * 4


def test_dump_outputs_writes_the_last_steps_arrays(plain_run):
    _, d = plain_run
    shapes = {"kp2d": (N_CROPS, N_JOINTS, 2), "score": (N_CROPS, N_JOINTS), "argmax": (N_CROPS, N_JOINTS),
              "kp3d": (1, 4 * N_JOINTS, 3), "heatmaps": (N_CROPS, N_JOINTS, 64, 48)}
    assert sorted(os.listdir(d)) == sorted(f"{k}.npy" for k in shapes)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64e6
    a = {k: np.load(os.path.join(d, f"{k}.npy")) for k in shapes}
    for k, s in shapes.items():
        assert a[k].shape == s and a[k].dtype in (np.float32, np.float64), (k, a[k].shape, a[k].dtype)
    assert np.isfinite(a["kp2d"]).all() and np.isfinite(a["score"]).all() and np.isfinite(a["heatmaps"]).all()
    # the arrays belong together: argmax is the heatmap's peak cell, and the bench's scaled head puts points in 3D
    hm = a["heatmaps"].reshape(N_CROPS, N_JOINTS, -1)
    assert np.array_equal(a["argmax"], hm.argmax(-1).astype(np.float32))
    assert np.isfinite(a["kp3d"]).any()


def test_dump_outputs_repeat_with_the_same_arguments(plain_run, tmp_path):
    _, d = plain_run
    _run(tmp_path)
    for f in sorted(os.listdir(d)):
        a, b = np.load(os.path.join(d, f)), np.load(os.path.join(tmp_path, f))
        assert np.array_equal(a, b, equal_nan=True), f
