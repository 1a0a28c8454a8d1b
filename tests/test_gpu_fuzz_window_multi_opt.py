"""A seeded prefix of the randomised sweep of the multi-target windows' summed objective (tests/fuzz/fuzz_window_multi_opt.py:
the generator of fuzz_window_multi.py -- random kernel, N <= 200, P <= 64, d, up to six windows, a number of ticks from empty to
two turnovers in up to three pushes) against tests/window_multi_opt_oracle.py.  The case sequence of a seed is fixed and the prefix
is a number of cases, not a time: the first 30 cases of seed 1, of which the oracle alone
(python tests/fuzz/fuzz_window_multi_opt.py 600 1 30 oracle-only, no GPU) skips none -- the windows have no jitter ladder, so a
case whose oracle fit needs jitter would be skipped, and none may be skipped here."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_window_multi_opt_prefix():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_window_multi_opt.py"), "3000", "1", "30"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("cases 30 failures 0 skipped 0 "), last
