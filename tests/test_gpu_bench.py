"""bench.py as it is run for every change: a plain run prints the headline line only, and --dump-outputs writes what the timed
path's last step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_with_dumped_outputs(gpu, tmp_path):
    out = tmp_path / "outputs"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                           "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == 1, proc.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 5 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "Mpoints/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["points_per_gpu"] / line["ms_per_step"] / 1e3) <= 1e-6 * line["value"]
    for moved in ("roofline", "kernels", "config3", "config4", "config5", "call_then_count_us", "cpu_baseline", "parity"):
        assert moved not in line, moved
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"points_xyz", "points_rgb", "points_tile", "cellsize", "timestamp", "count"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    n = line["config"]["outputs_per_gpu"]
    assert n == 39548 and got["count"][0] == n and got["points_xyz"].shape == (n, 3) and got["points_rgb"].shape == (n, 3)
    assert got["cellsize"][0] > 0 and np.isfinite(got["points_xyz"]).all()
    rgb = got["points_rgb"]
    assert (rgb == np.round(rgb)).all() and rgb.min() >= 0 and rgb.max() <= 255 and (got["points_tile"] > 0).all()
