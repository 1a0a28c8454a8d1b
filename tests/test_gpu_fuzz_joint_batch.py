"""A seeded prefix of the randomised sweep of the joint forecast after batch fits (tests/fuzz/fuzz_joint_batch.py: covariances and
sample paths of random batches, all five kernels) against the refit oracle.  The case sequence of a seed is fixed and the prefix
is a number of cases, not a time: the first 30 cases of seed 1, on which the oracle alone (python tests/fuzz/fuzz_joint_batch.py
600 1 30 oracle-only, no GPU) raises no LinAlgError -- so none may be dropped here either."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_joint_batch_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_joint_batch.py"), "3000", "1", "30"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 30 failures 0 dropped 0 "), last
