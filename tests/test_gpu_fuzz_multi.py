"""A seeded prefix of the randomised sweep of the multi-target fits (tests/fuzz/fuzz_multi.py: random batches, all five kernels,
P targets per fit) against one oracle refit per column.  The case sequence of a seed is fixed and the prefix is a number of
cases, not a time: the first 16 cases of seed 1.  The sweep drops no case."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_multi_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_multi.py"), "3000", "1", "16"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 16 failures 0 "), last
