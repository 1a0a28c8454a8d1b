"""A seeded prefix of the randomised sweep of the leave-one-out objective (tests/fuzz/fuzz_loo_grad.py: random kernel, N <= 301,
d, batch <= 40) against tests/loo_grad_oracle.py.  The case sequence of a seed is fixed and the prefix is a number of cases, not a
time: the first 20 cases of seed 1, of which the oracle alone (python tests/fuzz/fuzz_loo_grad.py 600 1 20 oracle-only, no GPU)
skips none -- under the sweep's cap of one skipped case in ten, so none may be skipped here either."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_loo_grad_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_loo_grad.py"), "3000", "1", "20"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 20 failures 0 skipped 0 "), last
