"""A compiled ISO C11 caller of the sliding-window forecast (tests/c_abi/window_forecast.c: cgp_window_init -> cgp_window_push ->
cgp_window_predict), built `-pedantic -Werror` like the other callers; on the GPU it checks one forecast value against the number
this test computes with the oracle and passes on the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from forecast_oracle import sliding_window_forecast

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_forecast")), "window_forecast")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "window_forecast.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_forecast_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,M,j", [(40, 100, 599, 598), (64, 30, 20, 0)])
def test_c_caller_forecasts_from_a_window_on_the_gpu(caller, N, T, M, j):
    x = 11.0 + np.arange(T)
    y = 0.1 * np.sin(2.0 * np.pi * x / 40.0) + 0.02 * np.cos(0.7 * x)      # the caller's stream
    Xs = x[-1] + 1.0 + np.arange(M)
    mu, var = sliding_window_forecast(2, np.array([0.5, 30.0, 0.01, 0.002]), N, x[:, None], y, Xs[:, None])
    r = subprocess.run([caller, str(N), str(T), str(M), str(j), repr(float(mu[j])), repr(float(var[j]))], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "window_forecast.c ok" in r.stdout
