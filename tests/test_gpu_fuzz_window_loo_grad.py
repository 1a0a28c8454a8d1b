"""A seeded prefix of the randomised sweep of the windows' leave-one-out objective (tests/fuzz/fuzz_window_loo_grad.py: random
kernel, N, d, windows, pushes and set_theta interleaved) against tests/window_loo_grad_oracle.py.  The case sequence of a seed is
fixed and the prefix is a number of cases, not a time: the first 30 cases of seed 1, of which the oracle alone (python
tests/fuzz/fuzz_window_loo_grad.py 600 1 30 oracle-only, no GPU) skips none, so none may be skipped here either."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_window_loo_grad_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_window_loo_grad.py"), "3000", "1", "30"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 30 failures 0 skipped 0 "), last
