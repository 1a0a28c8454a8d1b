"""tools/bench_matern.py prints ONE JSON line that sets the Matern kernels beside SE_ARD on identical samples (full batch, mid-size
call, window push / forecast, the 134-sample node callback): its keys exist and are finite, and the outputs it timed passed its
in-run check against the test oracle."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matern_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_matern.py"), "--full", "24", "--mid", "8", "--windows", "64",
                        "--reps", "2", "--ticks", "16"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    ex = json.loads(lines[0])
    for name in ("se_ard", "matern32", "matern52"):
        for k in ("full_ms", "full_fits_per_s", "mid_ms", "push_us_per_tick", "forecast_ms", "node_ms", "node_opt_ms", "node_opt_evals"):
            v = ex[f"{k}_{name}"]
            assert math.isfinite(v) and v > 0, (k, name, v)
    for k in ("full", "mid", "push_us_per_tick", "forecast_ms"):
        for name in ("matern32", "matern52"):
            assert 0.2 < ex[f"{k}_{name}_over_se_ard"] < 5.0, (k, name, ex)
    assert 0 <= ex["max_rel_err_vs_oracle"] < 1e-6
    assert ex["full_fits"] == 24 and ex["mid_fits"] == 8 and ex["windows"] == 64 and ex["value"] > 0
