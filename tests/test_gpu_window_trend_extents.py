"""The extents of every caller buffer of cgp_window_predict_trend_device on guard-band allocations (tests/guarded.py), by the
method and with the machinery of tests/test_gpu_device_extents.py (its docstring states what is asserted: nothing outside the
documented extents written, every documented element written, results independent of guard content and of element alignment, a
failed window beside healthy ones).  M and the column counts are no multiples of 16 or 128: the kernels work in 16-column tiles
and 128 test points per workgroup."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_device_extents as ext
from test_gpu_device_extents import F64, I32, R, IN, Case, check_case, win_data, pre_ticks, ids
import trend_oracle as to

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


def basis_of(x0, q):
    """[1, u, u^2][:q] of win_data's first input (already standardised over the stream)."""
    return np.stack([to.basis(x, 0.0, 1.0, q) for x in x0])      # (W, q, len)


@functools.lru_cache(maxsize=None)
def columns(W, N, d, Pt, q):
    """The pushed columns on win_data's streams: Pt targets (column 0 is its y), then the q basis columns."""
    X, y, _ = win_data(W, N, d)
    rng = np.random.default_rng(N + Pt)
    Y = np.stack([y] + [y * (1.0 + 0.3 * p) + rng.normal(0, 0.01, y.shape) for p in range(1, Pt)], axis=2)
    return np.concatenate([Y, basis_of(X[:, :, 0], q).transpose(0, 2, 1)], axis=2)


def setup(ctx, W, N, d, Pt, q, M, state, fail=False):
    X, _, theta = win_data(W, N, d)
    Y = columns(W, N, d, Pt, q)
    pre = pre_ticks(N, state)
    ctx.window_init(W, N, d, ext.WKID, theta)
    ctx.window_multi_reserve(Pt + q)
    ctx.window_trend_reserve(q, M)      # exactly M
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


@pytest.mark.parametrize("M,Pt,q", [(1, 1, 1), (17, 3, 2), (33, 15, 3), (130, 2, 3)])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_predict_trend_device(wctx, wnd, state, M, Pt, q):
    W, N, d = wnd

    def build(mode):
        Xs = np.resize(ext.forecast_points(W, N, d, state, min(M, 40)), (W, M, d)) if M > 40 else ext.forecast_points(W, N, d, state, M)
        regs = [IN("dxs", F64, Xs), IN("dHs", F64, basis_of(Xs[:, :, 0], q)), R("dmean", F64, (W, Pt, M), nan=True),
                R("dvar", F64, (W, M), nan=True), R("dbeta", F64, (W, Pt, q), nan=True), R("dlogml", F64, (W, Pt), nan=True),
                R("dtinfo", I32, (W,))]

        def call(p):
            setup(wctx, W, N, d, Pt, q, M, state, fail=mode == "fail")
            assert wctx.window_predict_trend_device(M, Pt + q, q, p["dxs"], p["dHs"], True, p["dmean"], p["dvar"], p["dbeta"],
                                                    p["dlogml"], p["dtinfo"], 0) == 0
        return Case(regs, call, zero=("dtinfo",))
    check_case(build)
