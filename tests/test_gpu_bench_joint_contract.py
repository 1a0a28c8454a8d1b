"""tools/bench_window_joint.py prints ONE JSON line about the windows' joint forecast (covariance and sample paths) beside the
marginal forecast and a refit: its keys exist and are finite, and the outputs it timed agree with the refit oracle."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_joint_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_window_joint.py"), "--windows", "128", "--reps", "2", "--m", "100", "64"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    ex = json.loads(lines[0])
    for sfx in ("", "_m64"):
        for k in ("window_joint_cov_ms", "window_joint_sample_ms", "window_joint_cov_frac_of_fp64_mfma_peak",
                  "window_joint_sample_frac_of_fp64_mfma_peak", "window_joint_marginal_ms", "window_joint_refit_ms"):
            assert k + sfx in ex and math.isfinite(ex[k + sfx]) and ex[k + sfx] > 0, (k + sfx, ex.get(k + sfx))
        assert 0 <= ex["window_joint_max_rel_err_vs_oracle" + sfx] < 1e-6, ex
        # the joint calls contain the marginal forecast's solve
        assert ex["window_joint_sample_ms" + sfx] > 0.5 * ex["window_joint_marginal_ms" + sfx]
    assert ex["windows"] == 128 and ex["N"] == 512 and ex["paths"] == 16 and ex["value"] > 0
