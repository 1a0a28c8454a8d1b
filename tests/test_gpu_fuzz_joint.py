"""A short prefix of the randomised sweep of the sliding windows' joint forecast (tests/fuzz/fuzz_window_joint.py: pushes,
covariances and sample paths at random moments of random streams) against the refit oracle.  The seeded case sequence is fixed;
the time budget only decides how long a prefix of it runs."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_window_joint_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_window_joint.py"), "15", "1"], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases ") and " failures 0 " in last, last
    assert int(last.split()[1]) >= 5, last
