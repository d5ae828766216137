"""bench.py as the project's yardstick runs it (pytest -m gpu): a plain run times exactly --steps steps, prints the headline
fields and nothing from --full, and --dump-outputs writes the timed path's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_times_the_given_steps_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "Msplats/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    for k in ("stage_ms", "roofline", "cpu_baseline", "literal_t_min_0", "train_iteration", "ms_per_step_unsettled"):
        assert k not in d, k
    n, W, H = 10000, 256, 256                                     # C1, SH degree 0
    shapes = {"d_means": (n, 3), "d_scales": (n, 3), "d_quaternions": (n, 4), "d_opacities": (n, 1), "d_shs": (n, 3),
              "image": (3, H, W), "transmittance": (H, W)}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in shapes)
    for k, shape in shapes.items():
        a = np.load(out / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), k
    assert np.abs(np.load(out / "d_means.npy")).max() > 0 and np.load(out / "image.npy").max() > 0
