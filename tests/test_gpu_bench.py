"""``bench.py`` as every change runs it: the plain run reports the timed steps only, and ``--dump-outputs`` writes what
the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_reports_the_timed_steps_and_dumps_the_last_one(tmp_path):
    out_dir = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2",
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 6 and line["unit"] == "graphs/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - 1024 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    assert line["full"] is False
    for key in ("kernels", "roofline", "lightpath", "reference_scale", "cpu_baseline", "ms_per_step_median"):
        assert key not in line, key                  # measured with --full only

    names = sorted(f[:-4] for f in os.listdir(out_dir) if f.endswith(".npy"))
    assert "out" in names and "loss" in names and "param.conv2.nn.2.weight" in names, names
    arrays = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["out"].shape == (1024, 3)
    assert arrays["loss"].shape == () and float(arrays["loss"]) == pytest.approx(line["config"]["final_loss"], rel=1e-6)
