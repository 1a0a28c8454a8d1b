"""A compiled ISO C11 caller of the windows' hyper-parameters replaced in place (tests/c_abi/window_adapt.c: cgp_window_init ->
cgp_window_push -> cgp_window_set_theta -> cgp_window_nll_grad -> cgp_window_optimize), built `-pedantic -Werror` like the other
callers; on the GPU it checks logML and one gradient entry against the numbers this test computes with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from adapt_oracle import window_nll_grad

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_adapt")), "window_adapt")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "window_adapt.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_adapt_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_five_symbols_are_declared_and_bound():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in ("cgp_window_set_theta", "cgp_window_set_theta_device", "cgp_window_nll_grad", "cgp_window_nll_grad_device",
                 "cgp_window_optimize"):
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_ABI_VERSION 3" in hdr


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(40, 100), (64, 30)])
def test_c_caller_changes_theta_of_a_window_on_the_gpu(caller, N, T):
    x = 11.0 + np.arange(T)
    y = 0.1 * np.sin(2.0 * np.pi * x / 40.0) + 0.02 * np.cos(0.7 * x)      # the caller's stream
    nll, g = window_nll_grad(2, np.array([0.8, 45.0, 0.02, 0.004]), N, x[:, None], y, T)
    r = subprocess.run([caller, str(N), str(T), repr(float(-nll)), repr(float(g[0]))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "window_adapt.c ok" in r.stdout
