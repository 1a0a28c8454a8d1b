"""tools/bench_window_forecast.py prints ONE JSON line about the sliding windows' forecast: its keys exist and are finite, the
timed call's outputs agree with the refit oracle, and the M = 64 forecast beats the refit route on the same windows."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forecast_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_window_forecast.py")], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    ex = json.loads(lines[0])
    for k in ("window_forecasts_per_s", "window_forecast_ms", "window_forecast_frac_of_fp64_mfma_peak", "window_forecast_hbm_frac",
              "window_forecast_host_ms_one_window", "window_forecast_vs_refit", "window_forecast_vs_refit_m64",
              "window_forecast_ms_m64", "window_forecast_max_rel_err_vs_oracle", "window_forecast_max_rel_err_vs_oracle_m64"):
        assert k in ex and math.isfinite(ex[k]) and ex[k] > 0, (k, ex.get(k))
    assert ex["window_forecast_max_rel_err_vs_oracle"] < 1e-6 and ex["window_forecast_max_rel_err_vs_oracle_m64"] < 1e-6
    assert ex["window_forecast_vs_refit_m64"] > 1.0, ex["window_forecast_vs_refit_m64"]
    assert ex["window_ticks_per_s"] > 0 and ex["windows"] == 1024 and ex["N"] == 512
