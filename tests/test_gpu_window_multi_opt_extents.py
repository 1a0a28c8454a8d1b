"""The extents of every caller buffer of cgp_window_multi_nll_grad_device on guard-band allocations (tests/guarded.py), by the
method and with the machinery of tests/test_gpu_device_extents.py (its docstring states what is asserted: nothing outside the
documented extents written -- the gap columns [ntheta, grad_stride) of the gradient included --, every documented element written,
logml given or NULL, results independent of guard content and of element alignment, a failed window beside healthy ones).  P is
no multiple of 16: the kernels work in 16-column target tiles."""
import numpy as np
import pytest

import test_gpu_device_extents as ext
from test_gpu_device_extents import F64, R, Case, check_case, ids
from test_gpu_window_multi_extents import WIN, STATES, setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


@pytest.fixture(scope="module")
def wctx(engine):
    c = engine.Context(max_n=8, max_m=8, max_d=2)       # the windows bring their own buffers
    yield c
    c.close()


@pytest.mark.parametrize("P,extra", [(1, 0), (3, 3), (17, 0)])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_multi_nll_grad_device(wctx, wnd, state, P, extra):
    W, N, d = wnd
    nth, stride = d + 2, d + 2 + extra

    def build(mode):
        regs = [R("dnll", F64, (W,), nan=True), R("dgrad", F64, (W, stride), keep=np.arange(stride) >= nth, nan=True),
                R("dlogml", F64, (W, P), nan=True, optional=True)]

        def call(p):
            setup(wctx, W, N, d, P, state, fail=mode == "fail")
            wctx.window_multi_grad_reserve()
            assert wctx.window_multi_nll_grad_device(P, p["dnll"], p["dgrad"], stride, p["dlogml"], 0) == 0
        return Case(regs, call)
    check_case(build)
