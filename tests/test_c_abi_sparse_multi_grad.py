"""A compiled ISO C11 caller of the sparse fits' objective with P target columns (tests/c_abi/sparse_multi_grad.c:
cgp_sparse_multi_grad_reserve, cgp_sparse_multi_nll_grad_batch, cgp_optimize_sparse_multi_batch), built `-pedantic -Werror` like the
other callers; on the GPU it checks the status codes, the N = 1, m = 1 gradient of two columns against the closed-form bound
differentiated by central differences in long double, P identical columns against P times the single-column call within 1e-9, and
one joint optimiser run."""
import os
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")
SYMBOLS = ("cgp_sparse_multi_grad_reserve", "cgp_sparse_multi_nll_grad_batch", "cgp_sparse_multi_nll_grad_batch_device",
           "cgp_optimize_sparse_multi_batch")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_sparse_multi_grad")), "sparse_multi_grad")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "sparse_multi_grad.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_sparse_multi_grad_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_symbols_are_declared_and_bound():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_ABI_VERSION 3" in hdr and "#define CGP_PROF_KERNELS 5" in hdr


@pytest.mark.gpu
def test_c_caller_checks_status_closed_form_gradient_identical_columns_and_the_optimiser_on_the_gpu(caller):
    r = subprocess.run([caller], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "sparse_multi_grad.c ok" in r.stdout
