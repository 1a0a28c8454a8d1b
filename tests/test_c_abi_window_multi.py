"""A compiled ISO C11 caller of the multi-target sliding windows (tests/c_abi/window_multi.c: cgp_window_multi_reserve,
cgp_window_push_multi and cgp_window_predict_multi on an empty window, after one pushed tick and after four), built
`-pedantic -Werror` like the other callers; on the GPU it checks the prior, the n = 1 closed form and the linearity of the mean in
the targets, which the C file writes out itself, for SE-ARD and RBF x Brownian.  The symbol checks need no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")
SYMBOLS = ("cgp_window_multi_reserve", "cgp_window_push_multi", "cgp_window_push_multi_device", "cgp_window_predict_multi",
           "cgp_window_predict_multi_device")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_window_multi")), "window_multi")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "window_multi.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_window_multi_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_five_symbols_are_declared_bound_and_exported():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_ABI_VERSION 3" in hdr
    assert "multi-target sliding windows, and" not in hdr   # (the "Not provided" sentence of the batch multi-target section)
    lib = engine.load()   # binds every symbol of EXPORTS from the library built for gfx950, or raises
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.cgp_abi_version() == 3


@pytest.mark.gpu
def test_c_caller_checks_the_prior_the_n1_closed_form_and_linearity_on_the_gpu(caller):
    r = subprocess.run([caller], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "window_multi.c ok" in r.stdout
