"""A compiled ISO C11 caller of the Matern kernels (tests/c_abi/matern.c: cgp_fit -> cgp_predict -> cgp_nll_grad), built
`-pedantic -Werror` like the other callers; on the GPU it checks every output against the closed forms of
tests/golden/matern_closed_m{32,52}_n2.npz."""
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
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_matern")), "matern")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "matern.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_matern_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["m32", "m52"])
def test_c_caller_matern_closed_form_on_the_gpu(caller, tmp_path, tag):
    g = load_golden(f"matern_closed_{tag}_n2")
    parts = [g["theta"], g["X"], g["y"], g["Xs"], g["mean"], g["var_latent"], g["logml"], g["dlogml_dtheta"]]
    path = os.path.join(str(tmp_path), "matern.txt")
    with open(path, "w") as f:
        f.write(f"{int(g['kernel_id'])}\n" + "\n".join(repr(float(v)) for p in parts for v in np.asarray(p, dtype=np.float64).ravel()) + "\n")
    r = subprocess.run([caller, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "matern.c ok" in r.stdout
