"""A seeded prefix of the randomised sweep of the sparse fits' objective with P target columns
(tests/fuzz/fuzz_sparse_multi_grad.py: fuzz_sparse_grad.py's cases with a random column count, against the one-factor statement of
tests/sparse_multi_grad_oracle.py and, bitwise, the multi-column forward call and the single-column gradient call).  The case
sequence of a seed is fixed and the prefix is a number of accepted cases, not a time: the first 8 of seed 1.  The sweep compares
only inputs that meet the oracle's own conditions, counts the draws it rejects and fails when more than 10 % are."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_sparse_multi_grad_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_sparse_multi_grad.py"), "3000", "1", "8"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout[-600:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("cases 8 failures 0 "), lines[-1]
    drawn, rejected = int(lines[-2].split()[1]), int(lines[-2].split()[3])
    assert rejected <= 0.1 * drawn, lines[-2]
