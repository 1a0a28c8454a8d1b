"""tools/bench_window_adapt.py prints ONE JSON line about the windows' set_theta / nll_grad / optimize beside the routes they
replace: its keys exist and are finite, and the outputs it timed agree with the refit oracle."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapt_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_window_adapt.py"), "--windows", "256", "--reps", "3", "--evals", "3"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    ex = json.loads(lines[0])
    for k in ("window_set_theta_ms", "window_set_theta_frac_of_fp64_mfma_peak", "window_nll_grad_ms", "window_nll_grad_frac_of_fp64_mfma_peak",
              "window_optimize_ms", "window_optimize_evals", "window_optimize_ms_per_eval", "window_set_theta_refit_ms",
              "window_set_theta_vs_refit", "batch_optimize_ms", "batch_optimize_ms_per_eval", "window_optimize_vs_batch",
              "reinit_repush_ms", "window_optimize_vs_repush", "window_set_theta_vs_repush", "value"):
        assert k in ex and math.isfinite(ex[k]) and ex[k] > 0, (k, ex.get(k))
    for k in ("window_set_theta_max_rel_err_vs_oracle", "window_nll_max_rel_err_vs_oracle", "window_grad_max_rel_err_vs_oracle"):
        assert 0 <= ex[k] < 1e-6, (k, ex[k])
    assert ex["windows"] == 256 and ex["N"] == 512 and 1 <= ex["window_optimize_evals"] <= 3
    # changing theta in place must beat initialising the windows again and pushing their N ticks back in
    assert ex["window_set_theta_vs_repush"] > 1.0, ex
