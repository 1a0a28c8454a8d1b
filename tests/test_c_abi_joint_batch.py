"""A compiled ISO C11 caller of the joint forecast after batch / single fits (tests/c_abi/joint_batch.c: cgp_joint_reserve ->
cgp_fit_predict_cov_batch -> cgp_fit_sample_batch -> cgp_fit -> cgp_predict_cov -> cgp_sample), built `-pedantic -Werror` like the
other callers; on the GPU it checks every output against tests/golden/closed_joint_n2_se.npz (a closed form)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_joint_batch")), "joint_batch")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "joint_batch.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_joint_batch_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


@pytest.mark.gpu
def test_c_caller_joint_batch_on_the_gpu(caller, tmp_path):
    g = load_golden("closed_joint_n2_se")
    S, M = g["xi"].shape
    parts = [g["theta"], g["X"], g["y"], g["Xs"], g["xi"], g["jitter_rel"], g["mean"], g["cov_latent"], g["noise"], g["paths"]]
    path = os.path.join(str(tmp_path), "joint.txt")
    with open(path, "w") as f:
        f.write(f"{M} {S}\n" + "\n".join(repr(float(v)) for p in parts for v in np.asarray(p, dtype=np.float64).ravel()) + "\n")
    r = subprocess.run([caller, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "joint_batch.c ok" in r.stdout
