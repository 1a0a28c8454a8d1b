"""A short prefix of the randomised sweep of the Matern kernels (tests/fuzz/fuzz_matern.py: random kernel, shape, batch, theta,
dense and sparse grids) against tests/matern_oracle.py.  The seeded case sequence is fixed; the time budget only decides how long
a prefix of it runs."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_matern_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_matern.py"), "60", "1"], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases ") and " failures 0 " in last, last
    assert int(last.split()[1]) >= 5, last
