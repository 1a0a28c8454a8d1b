"""The extents of every caller buffer of cgp_loo_nll_grad_batch_device on guard-band allocations (tests/guarded.py), by the method
and with the machinery of tests/test_gpu_device_extents.py (its docstring states what is asserted: nothing outside the documented
extents written -- the gap columns [ntheta, grad_stride) of the gradient included --, every documented element written, dlogml
given or NULL, results independent of guard content and of element alignment, a failed fit beside healthy ones).  Shapes are
test_loo_batch_device's: inside one tile, one row into the second, one row into the third."""
import numpy as np
import pytest

from test_gpu_device_extents import F64, I32, R, Case, check_case, fit_regions, ids, jit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


@pytest.fixture(scope="module")
def ctx64(engine):
    c = engine.Context(max_n=257, max_m=257, max_d=3, max_batch=3)
    assert c.loo_grad_reserve(3) == 0
    yield c
    c.close()


@pytest.mark.parametrize("d,extra", [(1, 0), (3, 3)])
@pytest.mark.parametrize("BN", [(3, 15), (3, 129), (2, 257)], ids=ids)
def test_loo_nll_grad_batch_device(ctx64, BN, d, extra):
    B, N = BN
    nth, stride = d + 2, d + 2 + extra

    def build(mode):
        regs = fit_regions(F64, B, N, d, 1, 1, mode)
        del regs[2]                # no test points
        regs += [R("dnlpd", F64, (B,), nan=True), R("dgrad", F64, (B, stride), keep=np.arange(stride) >= nth, nan=True),
                 R("dlogml", F64, (B,), optional=True), R("dinfo", I32, (B,))]

        def call(p):
            assert ctx64.loo_nll_grad_batch_device(B, N, d, 1, p["dX"], p["dy"], p["dtheta"], jit(p), p["dnlpd"], p["dgrad"], stride,
                                                   p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)
