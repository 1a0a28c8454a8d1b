"""The extents of every caller buffer of cgp_window_predict_gradients_device on guard-band allocations (tests/guarded.py), with the
machinery of test_gpu_device_extents.py (its module docstring states the four properties a .. d).  The kernel works in chunks of
32 test points, blocks of 16 samples and slabs rounded up to 16, while the header states the extents in real shapes: dmean_out /
dvar_out are exactly (nwin, M), ddmean / ddvar exactly (nwin, M, d).  Nothing outside them is written, every element of them is
written -- by empty and by failed windows too --, the inputs are untouched, the results depend neither on the guards' content nor
on an offset of one element; each of the four outputs may be NULL (one at a time here; the combinations are in
test_gpu_window_pgrad.py); a failed last window has NaN in its own rows and leaves its neighbours' bits alone.  The windows of a
context are pushed together and so share their size: empty, filling and full windows are three states of every case."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_device_extents as ex
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


@pytest.fixture(scope="module")
def ex_engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


@pytest.fixture(scope="module")
def wctx(ex_engine):
    c = ex_engine.Context(max_n=8, max_m=8, max_d=3)
    yield c
    c.close()


def pre_ticks(N, state):
    """Ticks pushed before the call: none, half a window, two windows and three ticks (full, slid, moved back once)."""
    return {"empty": 0, "filling": N // 2, "full": 2 * N + 3}[state]


@functools.lru_cache(maxsize=None)
def win_data(W, N, d, M, kid):
    """Streams of 2 N + 3 ticks per window, hyper-parameters of its own for every window, M test points per window (id 2: raw
    tick counts, the points half a tick apart from the middle of the last window on: ties, off-tick points and the grid after)."""
    T = 2 * N + 3
    rng = np.random.default_rng(900 + 10 * N + d + kid)
    t = np.arange(11, 11 + T, dtype=np.float64)
    X = np.empty((W, T, d))
    if kid == 2:
        X[:, :, 0] = t
        theta = np.tile([0.5, 30.0, 0.01, 0.002], (W, 1)) * rng.uniform(0.9, 1.1, (W, 1))
        Xs = np.repeat((t[-1] - N // 2 + 0.5 * np.arange(M, dtype=np.float64))[None, :, None], W, axis=0)
    else:
        X[:, :, 0] = (t - t.mean()) / t.std() * rng.uniform(0.8, 1.25, (W, 1))
        X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
        theta = np.column_stack([rng.uniform(0.01, 0.04, W), rng.uniform(0.8, 1.6, (W, d)), rng.uniform(0.5e-3, 2e-3, W)])
        Xs = X[:, rng.integers(T - N, T, size=M)] + 0.2 * rng.normal(size=(W, M, d))
    y = np.stack([synth._slip_series(rng, t) for _ in range(W)])
    return X, y, theta, Xs


def win_setup(ctx, W, N, d, M, kid, state, fail):
    """The resident state every run of a case starts from; for the failure runs the LAST window is failed by
    cgp_window_set_theta_device (sigma_n^2 = -2 sigma_f^2), as test_gpu_device_extents.win_setup does."""
    X, y, theta, _ = win_data(W, N, d, M, kid)
    pre = pre_ticks(N, state)
    ctx.window_init(W, N, d, kid, theta)
    if pre:
        ctx.window_push(X[:, :pre], y[:, :pre])
    if fail:
        bad = theta.copy()
        bad[-1, -1] = -2.0 * bad[-1, 0]
        dth = torch.from_numpy(bad).to(ex.DEV)
        dsel = torch.tensor([0] * (W - 1) + [1], dtype=U8, device=ex.DEV)
        di = torch.zeros(W, dtype=I32, device=ex.DEV)
        torch.cuda.synchronize()
        assert ctx.window_set_theta_device(dth.data_ptr(), theta.shape[1], dsel.data_ptr(), 0, di.data_ptr(), 0) == 0
        torch.cuda.synchronize()
        assert di[-1].item() != 0 and not di[:-1].any()


def pgrad_case(ctx, W, N, d, M, kid, state):
    def build(mode):
        if mode == "fail" and state == "empty":
            return None    # an empty window has no pivot to fail on
        regs = [ex.IN("dxs", F64, win_data(W, N, d, M, kid)[3]),
                ex.R("dmean", F64, (W, M), optional=True, nan=True), ex.R("dvar", F64, (W, M), optional=True, nan=True),
                ex.R("ddmean", F64, (W, M, d), optional=True, nan=True), ex.R("ddvar", F64, (W, M, d), optional=True, nan=True)]

        def call(p):
            win_setup(ctx, W, N, d, M, kid, state, fail=mode == "fail")
            assert ctx.window_predict_gradients_device(M, p["dxs"], True, p["dmean"], p["dvar"], p["ddmean"], p["ddvar"], 0) == 0
        return ex.Case(regs, call)
    return build


# (nwin, N, d, M, kid): a chunk and one point (M = 33) over a window of two blocks, the second half full, RBF x Brownian and
# SE-ARD at d = 3; three blocks and a single point with Matern 5/2
CASES = [(3, 24, 1, 33, 2), (3, 24, 3, 33, 1), (3, 40, 3, 1, 4)]


@pytest.mark.parametrize("state", ["empty", "filling", "full"])
@pytest.mark.parametrize("case", CASES, ids=ex.ids)
def test_window_predict_gradients_device(wctx, case, state):
    W, N, d, M, kid = case
    ex.check_case(pgrad_case(wctx, W, N, d, M, kid, state))
