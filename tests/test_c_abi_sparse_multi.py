"""A compiled ISO C11 caller of the sparse fits with P target columns (tests/c_abi/sparse_multi.c: cgp_sparse_multi_reserve,
cgp_fit_predict_sparse_multi_batch), built `-pedantic -Werror` like the other callers; on the GPU it checks the status codes, the
N = 1, m = 1 closed form of sparse.c for P = 2 targets and the linearity of the mean in Y, which the C file writes out itself."""
import os
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "c_abi")
LIBDIR = os.path.join(ROOT, "corenav_gp_amd")
SYMBOLS = ("cgp_sparse_multi_reserve", "cgp_fit_predict_sparse_multi_batch", "cgp_fit_predict_sparse_multi_batch_device")


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libcorenav_gp.so")):
        import __graft_entry__ as ge
        ge.build()
    exe = os.path.join(str(tmp_path_factory.mktemp("c_abi_sparse_multi")), "sparse_multi")
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "sparse_multi.c"), "-o", exe, "-L", LIBDIR, "-lcorenav_gp", "-lm",
                           f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_sparse_multi_caller_builds_and_links(caller):
    assert os.access(caller, os.X_OK)


def test_the_symbols_are_declared_and_bound():
    import corenav_gp_amd.engine as engine
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS
    assert "#define CGP_SPARSE_MAX_P 64" in hdr and "#define CGP_ABI_VERSION 3" in hdr


@pytest.mark.gpu
def test_c_caller_checks_status_closed_form_and_linearity_on_the_gpu(caller):
    r = subprocess.run([caller], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "sparse_multi.c ok" in r.stdout
