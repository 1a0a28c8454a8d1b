"""The extents of every caller buffer of cgp_window_push_multi_device and cgp_window_predict_multi_device on guard-band
allocations (tests/guarded.py), by the method and with the machinery of tests/test_gpu_device_extents.py (its docstring states
what is asserted: nothing outside the documented extents written, every documented element written, results independent of guard
content and of element alignment, an optional output omitted, a failed window beside healthy ones).  M and P are no multiples of
16: the kernels work in 16-column target tiles and 8 / 16 / 32 test points per workgroup."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_device_extents as ext
from test_gpu_device_extents import F64, R, IN, Case, check_case, win_data, pre_ticks, ids

pytestmark = pytest.mark.gpu

WIN = [(1, 17, 1), (3, 33, 2), (3, 130, 2)]
STATES = ext.STATES


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


@functools.lru_cache(maxsize=None)
def targets(W, N, d, P):
    """P target columns on win_data's streams: column 0 is its y."""
    _, y, _ = win_data(W, N, d)
    rng = np.random.default_rng(N + P)
    return np.stack([y] + [y * (1.0 + 0.3 * p) + rng.normal(0, 0.01, y.shape) for p in range(1, P)], axis=2)


def setup(ctx, W, N, d, P, state, fail=False):
    """win_setup of test_gpu_device_extents.py for a multi-target context: init, the reservation, `pre` ticks through the host
    push, and for the failure runs the LAST window failed by cgp_window_set_theta_device."""
    X, _, theta = win_data(W, N, d)
    Y = targets(W, N, d, P)
    pre = pre_ticks(N, state)
    ctx.window_init(W, N, d, ext.WKID, theta)
    ctx.window_multi_reserve(P)
    ctx.window_push_multi(X[:, :pre], Y[:, :pre])
    if fail:
        bad = theta.copy()
        bad[-1, -1] = -2.0 * bad[-1, 0]
        dth = torch.from_numpy(bad).to(ext.DEV)
        dsel = torch.tensor([0] * (W - 1) + [1], dtype=ext.U8, device=ext.DEV)
        di = torch.zeros(W, dtype=ext.I32, device=ext.DEV)
        torch.cuda.synchronize()
        assert ctx.window_set_theta_device(dth.data_ptr(), d + 2, dsel.data_ptr(), 0, di.data_ptr(), 0) == 0
        torch.cuda.synchronize()
        assert di[-1].item() != 0 and not di[:-1].any()
    return X, Y, pre


@pytest.mark.parametrize("T,P", [(1, 1), (3, 3), (5, 17)])
@pytest.mark.parametrize("state", STATES + ["compacting"])
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_push_multi_device(wctx, wnd, state, T, P):
    """(A push on a window that failed earlier still runs that window's ticks: its rows are only required to stay inside.)"""
    W, N, d = wnd

    def build(mode):
        X, pre = win_data(W, N, d)[0], pre_ticks(N, state)
        Y = targets(W, N, d, P)
        regs = [IN("dxs", F64, X[:, pre:pre + T]), IN("dYs", F64, Y[:, pre:pre + T]), R("dpm", F64, (W, T)), R("dpv", F64, (W, T)),
                R("dlm", F64, (W, T))]

        def call(p):
            setup(wctx, W, N, d, P, state, fail=mode == "fail")
            assert wctx.window_push_multi_device(T, P, p["dxs"], p["dYs"], True, p["dpm"], p["dpv"], p["dlm"], 0) == 0
        return Case(regs, call)
    check_case(build)


@pytest.mark.parametrize("M,P", [(1, 1), (17, 3), (33, 17)])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_predict_multi_device(wctx, wnd, state, M, P):
    W, N, d = wnd

    def build(mode):
        regs = [IN("dxs", F64, ext.forecast_points(W, N, d, state, M)), R("dmean", F64, (W, P, M), nan=True),
                R("dvar", F64, (W, M), nan=True), R("dlogml", F64, (W, P), nan=True, optional=True)]

        def call(p):
            setup(wctx, W, N, d, P, state, fail=mode == "fail")
            assert wctx.window_predict_multi_device(M, P, p["dxs"], True, p["dmean"], p["dvar"], p["dlogml"], 0) == 0
        return Case(regs, call)
    check_case(build)
