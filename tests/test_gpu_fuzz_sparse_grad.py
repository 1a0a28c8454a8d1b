"""A seeded prefix of the randomised sweep of the sparse fits' objective (tests/fuzz/fuzz_sparse_grad.py: random batches, all five
kernels, N across the chunks, m across the tiles and the row-tile groups, with and without gradZ) against
tests/sparse_grad_oracle.py.  The case sequence of a seed is fixed and the prefix is a number of accepted cases, not a time: the
first 12 of seed 1.  The sweep compares only inputs that meet the oracle's own conditions, counts the draws it rejects and fails
when more than 10 % are."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_sparse_grad_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_sparse_grad.py"), "3000", "1", "12"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-600:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("cases 12 failures 0 "), lines[-1]
    drawn, rejected = int(lines[-2].split()[1]), int(lines[-2].split()[3])
    assert rejected <= 0.1 * drawn, lines[-2]
