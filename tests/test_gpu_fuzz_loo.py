"""A seeded prefix of the randomised sweep of leave-one-out cross-validation after batch fits (tests/fuzz/fuzz_loo.py: random
kernel, N <= 400, d, batch <= 40) against tests/loo_oracle.py.  The case sequence of a seed is fixed and the prefix is a number
of cases, not a time: the first 40 cases of seed 1, of which the oracle alone (python tests/fuzz/fuzz_loo.py 600 1 40 oracle-only,
no GPU) skips none -- under the sweep's 5 % cap on skipped cases, so none may be skipped here either."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_loo_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_loo.py"), "3000", "1", "40"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 40 failures 0 skipped 0 "), last
