"""A seeded prefix of the randomised sweep of the multi-target objective (tests/fuzz/fuzz_multi_opt.py: random batches, all five
kernels, P targets per fit, both tile heights of the solve) against the per-column oracle.  The case sequence of a seed is fixed
and the prefix is a number of cases, not a time: the first 12 cases of seed 1.  The sweep drops no case."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_multi_opt_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_multi_opt.py"), "3000", "1", "12"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 12 failures 0 "), last
