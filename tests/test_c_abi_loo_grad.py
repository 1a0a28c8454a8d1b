"""A compiled ISO C11 caller of the leave-one-out objective (tests/c_abi/loo_grad.c: cgp_loo_grad_reserve, cgp_loo_nll_grad,
cgp_loo_nll_grad_batch), built `-pedantic -Werror` like the other callers; on the GPU it checks the N = 1 closed form and the N = 2
one against the 2 x 2 inverse, both of which the C file writes out itself."""
import os
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")
SYMBOLS = ("cgp_loo_grad_reserve", "cgp_loo_nll_grad", "cgp_loo_nll_grad_batch", "cgp_loo_nll_grad_batch_device", "cgp_optimize_loo_batch")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_loo_grad")), "loo_grad")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "loo_grad.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_loo_grad_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_five_symbols_are_declared_and_bound():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_ABI_VERSION 3" in hdr


@pytest.mark.gpu
def test_c_caller_checks_the_closed_forms_on_the_gpu(caller):
    r = subprocess.run([caller], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "loo_grad.c ok" in r.stdout
