"""GPU parity of the sliding windows' multi-point forecast (cgp_window_predict: mean / variance at M test points from the
factor, z and inputs the pushes maintain) against the oracle, which refits the window's samples from scratch."""
import numpy as np
import pytest

from oracle import gp_oracle as go
from forecast_oracle import sliding_window_forecast
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def stream(T, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + T, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    X = np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)])
    return X, y


def theta_of(kid, d):
    return {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]),
            1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]


def points_for(kid, X, t, M, rng):
    """RBF x Brownian: the reference's grid (the ticks after the last sample); SE: points around the window's inputs."""
    if kid == 2:
        return X[t - 1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    lo = max(0, t - 50)
    return X[rng.integers(lo, max(t, 1), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def close(mean, var, omu, ovar, tol=TOL):
    assert np.max(np.abs(mean - omu)) <= tol * max(np.max(np.abs(omu)), 1e-12), np.max(np.abs(mean - omu)) / np.max(np.abs(omu))
    assert np.max(np.abs(var - ovar) / ovar) < tol, np.max(np.abs(var - ovar) / ovar)


@pytest.mark.parametrize("kid,N,d", [(2, 16, 1), (2, 40, 1), (0, 33, 2), (1, 64, 3), (1, 100, 6)])
def test_forecast_matches_refit_oracle(engine, kid, N, d):
    """Forecasts of M = 1, 37, 599 points at several moments of one stream: an empty window, while filling, at n = N exactly,
    one tick before the ring compacts (origin + n = capacity - 1), at the last tick before the compaction, the tick after it,
    and after the window has turned over twice."""
    T = 3 * N + 6
    X, y = stream(T, d, 100 + N)
    theta = theta_of(kid, d)
    rng = np.random.default_rng(N)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta)
    fed = 0
    for t in (0, 1, N // 2, N - 3, N, 2 * N - 1, 2 * N, 2 * N + 1, T):
        if t > fed:
            ctx.window_push(X[fed:t][None], y[fed:t][None])
            fed = t
        assert ctx.window_state(0) == (min(N, t), 0)
        for M in (1, 37, 599):
            Xs = points_for(kid, X, max(t, 1), M, rng)
            for noise in (True, False):
                mean, var = ctx.window_predict(Xs, include_noise=noise)
                assert mean.shape == var.shape == (1, M)
                omu, ovar = sliding_window_forecast(kid, theta, N, X[:t], y[:t], Xs, include_noise=noise)
                if t == 0:
                    assert np.all(mean == 0.0)
                    np.testing.assert_allclose(var[0], ovar, rtol=1e-14)
                else:
                    close(mean[0], var[0], omu, ovar)


def test_config4_window512_forecast_two_device_paths(engine):
    """configs[3] size: N = 512, d = 3 after 1 200 ticks, the reference's horizon length M = 599: against the refit oracle, and
    against cgp_fit_predict_batch on the same 512 samples (two device paths, fp64 both)."""
    N, d, T, M = 512, 3, 1200, 599
    X, y = stream(T, d, 7)
    theta = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])
    rng = np.random.default_rng(5)
    ctx = engine.Context(max_n=512, max_m=640, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, rng)
    mean, var = ctx.window_predict(Xs)
    omu, ovar = sliding_window_forecast(1, theta, N, X, y, Xs)
    close(mean[0], var[0], omu, ovar)
    rc, bm, bv, _, info = ctx.fit_predict_batch(X[None, T - N:], y[None, T - N:], Xs[None], theta[None], 1)
    assert rc == 0 and info[0] == 0
    close(mean[0], var[0], bm[0], bv[0], tol=1e-9)


@pytest.mark.parametrize("kid,N,d", [(2, 150, 1), (1, 64, 3)])
def test_forecast_of_next_sample_is_the_next_push(engine, kid, N, d):
    """From a FILLING window the forecast at the next sample's input is the next push's pred_mean / pred_var: two summation
    orders of the same quantity (a full window drops a sample first: compared through the oracle only)."""
    X, y = stream(N, d, 40 + N)
    theta = theta_of(kid, d)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta)
    fed = 0
    for t in (1, 7, 16, 17, N // 2, N - 1):
        if t > fed:
            ctx.window_push(X[fed:t][None], y[fed:t][None])
        mean, var = ctx.window_predict(X[t:t + 1])
        pm, pv, _ = ctx.window_push(X[t:t + 1][None], y[t:t + 1][None])
        fed = t + 1
        assert abs(mean[0, 0] - pm[0, 0]) <= 1e-9 * max(abs(pm[0, 0]), np.max(np.abs(y))), (t, mean, pm)
        assert abs(var[0, 0] - pv[0, 0]) <= 1e-9 * pv[0, 0], (t, var, pv)


def test_forecast_does_not_touch_the_windows(engine):
    """push A, forecast, push B = push A, push B on a second context, bitwise (outputs of B and a forecast after it)."""
    N, d, T = 48, 2, 170
    X, y = stream(T, d, 77)
    theta = theta_of(1, d)
    rng = np.random.default_rng(1)
    Xs = points_for(1, X, T, 70, rng)
    outs = []
    for forecast_between in (True, False):
        ctx = engine.Context(max_n=8, max_m=8, max_d=d)
        ctx.window_init(1, N, d, 1, theta)
        ctx.window_push(X[:90][None], y[:90][None])
        if forecast_between:
            ctx.window_predict(Xs)
            ctx.window_predict(Xs[:3], include_noise=False)
        outs.append(ctx.window_push(X[90:][None], y[90:][None]) + ctx.window_predict(Xs))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_many_windows_are_independent_of_slot_and_neighbours(engine):
    """600 windows x N = 64 with distinct theta and data (several rounds of workgroups per CU), M = 100: eight of them against
    the oracle; and a window's forecast bitwise equal to the same stream in a context of one and of two windows."""
    W, N, d, T, M = 600, 64, 2, 150, 100
    rng = np.random.default_rng(600)
    t = np.arange(11, 11 + T, dtype=np.float64)
    X = np.empty((W, T, d))
    X[:, :, 0] = (t - t.mean()) / t.std()
    X[:, :, 1] = rng.normal(size=(W, T))
    y = np.stack([synth._slip_series(rng, t) for _ in range(W)])
    theta = np.column_stack([0.02 + 0.01 * rng.random(W), 0.8 + rng.random(W), 0.8 + rng.random(W), 1e-3 * (1 + rng.random(W))])
    Xs = X[:, rng.integers(T - N, T, size=M)] + 0.3 * rng.normal(size=(W, M, d))
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, 1, theta)
    ctx.window_push(X, y)
    mean, var = ctx.window_predict(Xs)
    for w in (0, 1, 85, 171, 299, 300, 513, 599):
        omu, ovar = sliding_window_forecast(1, theta[w], N, X[w], y[w], Xs[w])
        close(mean[w], var[w], omu, ovar)
    # the pushes of a small context take other kernels than those of a large one (same arithmetic to rounding, not bitwise), so
    # the windows are brought to the same state tick by tick: one-tick pushes are the single-tick kernel whatever the context
    for ws in ([299], [513, 7]):
        big = engine.Context(max_n=8, max_m=8, max_d=d)
        big.window_init(W, N, d, 1, theta)
        small = engine.Context(max_n=8, max_m=8, max_d=d)
        small.window_init(len(ws), N, d, 1, theta[ws])
        for k in range(40):
            big.window_push(X[:, k:k + 1], y[:, k:k + 1])
            small.window_push(X[ws, k:k + 1], y[ws, k:k + 1])
        bm, bv = big.window_predict(Xs)
        sm, sv = small.window_predict(Xs[ws])
        assert np.array_equal(bm[ws], sm) and np.array_equal(bv[ws], sv)


def test_host_and_device_forms_agree_bitwise(engine):
    import torch
    W, N, d, T, M = 3, 40, 3, 100, 53
    rng = np.random.default_rng(9)
    Xw, yw = zip(*[stream(T, d, 500 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = theta_of(1, d)
    Xs = X[:, rng.integers(T - N, T, size=M)] + 0.2 * rng.normal(size=(W, M, d))
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, 1, theta)
    ctx.window_push(X, y)
    mean, var = ctx.window_predict(Xs)
    dxs = torch.from_numpy(Xs).cuda()
    for stream_arg in (0, engine.STREAM_CTX):
        dm = torch.full((W, M), -1.0, dtype=torch.float64, device="cuda")
        dv = torch.full((W, M), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.window_predict_device(M, dxs.data_ptr(), True, dm.data_ptr(), dv.data_ptr(), stream=stream_arg) == 0
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dv.cpu().numpy(), var)


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    buf = np.zeros(4)
    p = engine._p(buf)
    assert ctx.lib.cgp_window_predict(ctx.h, 1, p, 1, p, p) == ESTATE
    assert ctx.lib.cgp_window_predict_device(ctx.h, 1, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, None) == ESTATE
    ctx.window_init(1, 8, 1, 2, theta_of(2, 1))
    assert ctx.lib.cgp_window_predict(ctx.h, 0, p, 1, p, p) == EINVAL
    assert ctx.lib.cgp_window_predict(ctx.h, 1, None, 1, p, p) == EINVAL
    assert ctx.lib.cgp_window_predict(ctx.h, 1, p, 1, None, p) == EINVAL
    assert ctx.lib.cgp_window_predict_device(ctx.h, 1, buf.ctypes.data, 1, buf.ctypes.data, None, None) == EINVAL


def test_failed_window_answers_nan_and_the_others_are_unaffected(engine):
    """Window 1 of three has sigma_n^2 < -sigma_f^2: its first pivot is negative, which the push flags (a compare on the
    pivot, a numerical status).  The forecast returns the same code, NaN for that window and parity for the other two."""
    W, N, d, T, M = 3, 24, 1, 30, 40
    Xw, yw = zip(*[stream(T, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    theta[1, -1] = -2.0 * theta[1, 0]
    rng = np.random.default_rng(2)
    Xs = X[:, -1:, :] + rng.random((W, M, 1)) * 5.0
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, 0, theta)
    with pytest.raises(engine.CgpError):
        ctx.window_push(X, y)
    code = ctx.window_state(1)[1]
    assert code > 0 and ctx.window_state(0)[1] == 0 and ctx.window_state(2)[1] == 0
    mean, var, rc = ctx.window_predict(Xs, check=False)
    assert rc == code
    with pytest.raises(engine.CgpError):
        ctx.window_predict(Xs)
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    for w in (0, 2):
        omu, ovar = sliding_window_forecast(0, theta[w], N, X[w], y[w], Xs[w])
        close(mean[w], var[w], omu, ovar)


def test_long_window_form(engine):
    """N = 1 536: the form for windows longer than the LDS holds at full chunk width (correct, not fast)."""
    N, d, T, M = 1536, 2, 1700, 100
    X, y = stream(T, d, 1536)
    theta = theta_of(1, d)
    rng = np.random.default_rng(3)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, rng)
    mean, var = ctx.window_predict(Xs)
    omu, ovar = sliding_window_forecast(1, theta, N, X, y, Xs)
    close(mean[0], var[0], omu, ovar)


def test_mid_length_window_form(engine):
    """512 < N <= 1024 takes the one-tile form (sixteen test points per workgroup)."""
    N, d, T, M = 700, 3, 1500, 77
    X, y = stream(T, d, 700)
    theta = theta_of(1, d)
    rng = np.random.default_rng(4)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, rng)
    mean, var = ctx.window_predict(Xs)
    omu, ovar = sliding_window_forecast(1, theta, N, X, y, Xs)
    close(mean[0], var[0], omu, ovar)


def test_forecast_feeds_the_stop_time_lookahead(engine):
    """The streaming node end to end: windows fed the synthetic rover's slip, forecast 599 ticks ahead, sigma = 2 sqrt(var),
    into cgp_predict_stop_batch; fired / i / stop_cmd equal the oracle's look-ahead on the oracle's forecast."""
    W, N, M = 4, 149, 599
    theta = theta_of(2, 1)
    tw, sw = zip(*[synth.reference_window(n=200, tick0=11 + 3 * w, seed=4000 + w) for w in range(W)])
    X, y = np.stack(tw)[:, :, None], np.stack(sw)
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    ctx.window_init(W, N, 1, 2, theta)
    ctx.window_push(X, y)
    Xs = X[:, -1:, :] + 1.0 + np.arange(M, dtype=np.float64)[None, :, None]
    mean, var = ctx.window_predict(Xs)
    sigma = 2.0 * np.sqrt(var)
    states = [synth.filter_state(2000 + 31 * w) for w in range(W)]
    P, Q, STM, Hv, pos = (np.stack([s[j] for s in states]) for j in range(5))
    fired, cmd, iout, xy = ctx.predict_stop_batch(mean, sigma, P, Q, STM, Hv, pos, 50.0, 50.2)
    for w in range(W):
        omu, ovar = sliding_window_forecast(2, theta, N, X[w], y[w], Xs[w])
        close(mean[w], var[w], omu, ovar)
        ef, ec, ei, exy = go.predict_stop(omu, 2.0 * np.sqrt(ovar), P[w], Q[w], STM[w], go.unpack_H(Hv[w], True), pos[w], 50.0, 50.2)
        assert bool(fired[w]) == ef and iout[w] == ei
        assert cmd[w] == pytest.approx(ec, rel=1e-12) and xy[w] == pytest.approx(exy, rel=1e-6)
