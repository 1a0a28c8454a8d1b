"""A compiled ISO C11 caller of the multi-target windows' summed objective (tests/c_abi/window_multi_opt.c:
cgp_window_multi_grad_reserve, cgp_window_multi_nll_grad and cgp_window_optimize_multi on an empty window, after one pushed tick
and after four), built `-pedantic -Werror` like the other callers; on the GPU it checks the n = 1 closed form of the value and its
gradient and the linearity in duplicated columns, which the C file writes out itself, for SE-ARD and RBF x Brownian.  The symbol
checks need no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")
SYMBOLS = ("cgp_window_multi_grad_reserve", "cgp_window_multi_nll_grad", "cgp_window_multi_nll_grad_device",
           "cgp_window_optimize_multi")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_window_multi_opt")), "window_multi_opt")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "window_multi_opt.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_window_multi_opt_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_four_symbols_are_declared_bound_and_exported():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_ABI_VERSION 3" in hdr
    assert "Not provided: a multi-target window optimiser" not in hdr
    lib = engine.load()   # binds every symbol of EXPORTS from the library built for gfx950, or raises
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.cgp_abi_version() == 3


@pytest.mark.gpu
def test_c_caller_checks_the_n1_closed_form_and_linearity_on_the_gpu(caller):
    r = subprocess.run([caller], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "window_multi_opt.c ok" in r.stdout
