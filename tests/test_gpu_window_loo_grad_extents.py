"""cgp_window_loo_nll_grad_device on guard-band allocations, with the machinery and the window cases of
tests/test_gpu_device_extents.py: nothing outside the documented extents is written, every documented element is written, a
grad_stride above ntheta keeps the gap columns, dlogml may be NULL, and a failed window beside healthy ones answers NaN while its
neighbours keep their bits."""
import numpy as np
import pytest

from test_gpu_device_extents import F64, R, Case, WIN, STATES, check_case, ids, win_setup, engine, wctx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_loo_nll_grad_device(wctx, wnd, state, extra):
    W, N, d = wnd
    nth, stride = d + 2, d + 2 + extra

    def build(mode):
        regs = [R("dnlpd", F64, (W,), nan=True), R("dgrad", F64, (W, stride), keep=np.arange(stride) >= nth, nan=True),
                R("dlogml", F64, (W,), optional=True, nan=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail")   # (cgp_window_init drops the reservation)
            assert wctx.window_loo_grad_reserve() == 0
            assert wctx.window_loo_nll_grad_device(p["dnlpd"], p["dgrad"], stride, p["dlogml"], 0) == 0
        return Case(regs, call)
    check_case(build)
