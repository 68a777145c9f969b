"""bench.py's plain run, its --full run and --dump-outputs: a plain run prints the headline line without the secondary figures,
--full adds them, and two runs with the same arguments dump the same outputs of their last timed step (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--preroll-steps", "2", "--gaussians", "20000", "--width", "320",
         "--height", "192"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "step_ms")
FULL_ONLY = ("roofline", "kernels_ms_per_view", "launches_per_view", "fp32_variant", "views_in_flight_2", "batched_2_views")


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    _bench("--dump-outputs", str(b))
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY + ("cpu_baseline",):
        assert k not in d, k
    assert d["steps"] == 3 and d["full"] is False
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    for n in ("render", "render_gaussian_features", "depth", "radii", "grad_xyz", "grad_features_rest", "grad_opacity",
              "grad_viewspace_points"):
        assert n + ".npy" in names, n
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        assert np.array_equal(x, y), f"{n}: the two runs differ"
        total += x.nbytes
    assert total <= 64 * 10 ** 6
    img = np.load(a / "render.npy")
    assert img.shape == (3, 192, 320) and img.max() > 0
    assert np.abs(np.load(a / "grad_xyz.npy")).sum() > 0


def test_full_run_adds_the_secondary_figures():
    d = _bench("--full", "--no-cpu-baseline")
    for k in HEADLINE + FULL_ONLY:
        assert k in d, k
    assert d["full"] is True
    assert d["roofline"]["kernel_ms"] > 0 and d["kernels_ms_per_view"]
