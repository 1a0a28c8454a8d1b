"""The batched L-BFGS driver (corenav_gp_amd/csrc/lbfgs.hpp: lbfgs_minimize_logexp_batch) as a stand-alone C++ program built
with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own: lbfgs_batch_driver.cpp holds the
checks (every selected problem bitwise the run of lbfgs_minimize alone, one callback per round, no finished or unselected
problem marked active, the unselected theta untouched, the last-point-was-best flag)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def test_lbfgs_batch_driver_matches_single_runs(tmp_path):
    exe = str(tmp_path / "lbfgs_batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "corenav_gp_amd", "csrc"),
                           os.path.join(HERE, "lbfgs_batch_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.strip().endswith("ok"), r.stdout
