"""GPU tests of the hyper-parameters of the resident sliding windows replaced and re-estimated in place: cgp_window_set_theta
(new theta -> factor rebuilt from the resident samples), cgp_window_nll_grad (value and gradient from the resident factor) and
cgp_window_optimize (L-BFGS over the windows), against the refit oracle (tests/adapt_oracle.py on top of oracle/gp_oracle.py)."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
from adapt_oracle import stream_ticks, window_logml, window_nll_grad, window_of
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


def other_theta(kid, d, k=0):
    """A theta clearly away from theta_of (another amplitude, other length-scales, more noise); k varies it."""
    s = 1.0 + 0.15 * k
    return {2: np.array([0.8 * s, 45.0 / s, 0.02, 0.004 * s]), 0: np.array([0.05 * s, 0.6 * s, 3e-3]),
            1: np.concatenate([[0.05 * s], np.linspace(1.7, 0.6, d) * s, [4e-3]])}[kid]


def points_for(kid, X, t, M, rng):
    if kid == 2:
        return X[t - 1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    lo = max(0, t - 50)
    return X[rng.integers(lo, max(t, 1), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def close(mean, var, omu, ovar, tol=TOL):
    assert np.max(np.abs(mean - omu)) <= tol * max(np.max(np.abs(omu)), 1e-12), np.max(np.abs(mean - omu)) / np.max(np.abs(omu))
    assert np.max(np.abs(var - ovar) / ovar) < tol, np.max(np.abs(var - ovar) / ovar)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def check_ticks(out, ref, tol=TOL):
    pm, pv, lm = out
    om, ov, ol = ref
    assert np.max(np.abs(pm - om)) <= tol * max(np.max(np.abs(om)), np.max(np.sqrt(ov))), (pm, om)
    assert np.max(np.abs(pv - ov) / ov) < tol
    assert np.max(np.abs(lm - ol) / np.maximum(np.abs(ol), 1.0)) < tol, (lm, ol)


# ---- cgp_window_set_theta ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,N,d", [(2, 40, 1), (0, 33, 2), (1, 64, 3), (1, 48, 6), (0, 16, 1)])
def test_set_theta_mid_stream_and_the_stream_continues_under_it(engine, kid, N, d):
    """A new theta while the window fills, when it is just full, either side of a ring compaction and after thousands of
    ticks: logML and a forecast against the refit oracle under the new theta, then the pushes that follow against the oracle's
    stream under the new theta on the same samples."""
    K = 7
    moments = [3, N // 2 + 8, N, 2 * N - 8, 2 * N, 2 * N + 8, 3 * N + 5, 2000 + N // 3]   # (a moment the K ticks have passed: as soon as possible)
    T = moments[-1] + K
    X, y = stream(T, d, 300 + N)
    rng = np.random.default_rng(N)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta_of(kid, d))
    fed = 0
    for k, t in enumerate(moments):
        t = max(t, fed)
        if t > fed:
            ctx.window_push(X[fed:t][None], y[fed:t][None])
            fed = t
        theta = other_theta(kid, d, k)
        logml, info = ctx.window_set_theta(theta)
        assert info[0] == 0 and ctx.window_state(0) == (min(N, t), 0)
        assert abs(logml[0] - window_logml(kid, theta, N, X, y, t)) <= TOL * abs(window_logml(kid, theta, N, X, y, t))
        Xs = points_for(kid, X, t, 37, rng)
        mean, var = ctx.window_predict(Xs)
        close(mean[0], var[0], *sliding_window_forecast(kid, theta, N, X[:t], y[:t], Xs))
        out = ctx.window_push(X[t:t + K][None], y[t:t + K][None])
        fed = t + K
        check_ticks([o[0] for o in out], stream_ticks(kid, theta, N, X, y, t, t + K))


def test_set_theta_on_the_configs3_window(engine):
    """N = 512, d = 3 after 1 200 ticks: the four-accumulator form at its full size, then forty more ticks."""
    N, d, T, K = 512, 3, 1200, 40
    X, y = stream(T + K, d, 7)
    theta = np.array([0.03, 1.3, 1.1, 1.2, 2e-3])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, np.array([0.02, 1.0, 1.4, 0.9, 1e-3]))
    ctx.window_push(X[None, :T], y[None, :T])
    logml, info = ctx.window_set_theta(theta)
    ref = window_logml(1, theta, N, X, y, T)
    assert info[0] == 0 and abs(logml[0] - ref) <= TOL * abs(ref)
    Xs = points_for(1, X, T, 64, np.random.default_rng(1))
    mean, var = ctx.window_predict(Xs)
    close(mean[0], var[0], *sliding_window_forecast(1, theta, N, X[:T], y[:T], Xs))
    out = ctx.window_push(X[None, T:], y[None, T:])
    sel = [0, 1, 2, K - 1]
    ref = [np.concatenate([stream_ticks(1, theta, N, X, y, T + i, T + i + 1)[j] for i in sel]) for j in range(3)]
    check_ticks([o[0][sel] for o in out], ref)


@pytest.mark.parametrize("N,d,T", [(1024, 2, 1100), (1536, 1, 1600)])
def test_set_theta_and_gradient_long_window_forms(engine, N, d, T):
    """The eight- and sixteen-accumulator forms of the refactor (N <= 1024, N <= 2048) and the gradient on such a window."""
    kid = 1 if d > 1 else 0
    X, y = stream(T + 3, d, N)
    theta = other_theta(kid, d)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta_of(kid, d))
    ctx.window_push(X[None, :T], y[None, :T])
    logml, info = ctx.window_set_theta(theta)
    onll, og = window_nll_grad(kid, theta, N, X, y, T)
    assert info[0] == 0 and abs(logml[0] + onll) <= TOL * abs(onll)
    nll, g = ctx.window_nll_grad()
    assert abs(nll[0] - onll) <= TOL * abs(onll) and np.max(np.abs(g[0] - og)) <= TOL * np.max(np.abs(og))
    out = ctx.window_push(X[None, T:], y[None, T:])
    check_ticks([o[0] for o in out], stream_ticks(kid, theta, N, X, y, T, T + 3))


def test_set_theta_with_the_theta_a_window_has_reproduces_the_streamed_state(engine):
    """After ten thousand rank-1 updates the refactor under the SAME theta describes the same matrix: logML, a forecast and the
    next pushes agree with the streamed state (a second context that never saw the call) to 1e-9."""
    N, d, T, K = 48, 3, 10000, 20
    X, y = stream(T + K, d, 5)
    theta = theta_of(1, d)
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(1, N, d, 1, theta)
        last = c.window_push(X[None, :T], y[None, :T])[2][0, -1]
    logml, info = a.window_set_theta(theta)
    assert info[0] == 0 and abs(logml[0] - last) <= 1e-9 * abs(last)
    Xs = points_for(1, X, T, 50, np.random.default_rng(0))
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs)
    assert rel(ma, mb) < 1e-9 and np.max(np.abs(va - vb) / vb) < 1e-9
    oa, ob = a.window_push(X[None, T:], y[None, T:]), b.window_push(X[None, T:], y[None, T:])
    for u, v in zip(oa, ob):
        assert np.max(np.abs(u - v) / np.maximum(np.abs(v), 1e-3)) < 1e-9


def test_unselected_windows_are_untouched_bitwise(engine):
    """Context a: set_theta on windows 0 and 2 only; context b never sees the call.  Later pushes and forecasts of windows 1 and 3
    are array_equal; windows 0 and 2 follow the oracle under their new theta."""
    W, N, d, T, K = 4, 40, 2, 130, 9
    Xw, yw = zip(*[stream(T + K, d, 50 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(1, d), (W, 1))
    new = np.stack([other_theta(1, d, w) for w in range(W)])
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 1, theta)
        c.window_push(X[:, :T], y[:, :T])
    sel = np.array([1, 0, 1, 0], dtype=bool)
    logml, info = a.window_set_theta(new, select=sel)
    assert np.all(info == 0) and np.all(logml[~sel] == 0.0)
    Xs = X[:, T - 20:T] + 0.1
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs)
    oa, ob = a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])
    for w in (1, 3):
        assert np.array_equal(ma[w], mb[w]) and np.array_equal(va[w], vb[w])
        for u, v in zip(oa, ob):
            assert np.array_equal(u[w], v[w])
    for w in (0, 2):
        assert abs(logml[w] - window_logml(1, new[w], N, X[w], y[w], T)) <= TOL * abs(logml[w])
        close(ma[w], va[w], *sliding_window_forecast(1, new[w], N, X[w, :T], y[w, :T], Xs[w]))
        check_ticks([o[w] for o in oa], stream_ticks(1, new[w], N, X[w], y[w], T, T + K))
        assert not np.array_equal(ma[w], mb[w])


def test_result_does_not_depend_on_slot_neighbours_or_select(engine):
    """600 windows, each with its own samples and its own new theta.  A second context holds them in reverse order and
    refactors a random two thirds of them: logML, the stored state as the next pushes and a forecast show it, and the gradient
    are bitwise those of the first context."""
    W, N, d, T, K = 600, 32, 2, 45, 4
    rng = np.random.default_rng(9)
    t = np.arange(11, 11 + T + K, dtype=np.float64)
    X = np.stack([np.column_stack([(t - t.mean()) / t.std(), rng.normal(size=T + K)]) for _ in range(W)])
    y = np.stack([synth._slip_series(rng, t) for _ in range(W)])
    theta = np.tile(theta_of(1, d), (W, 1))
    new = np.stack([other_theta(1, d, w % 7) * (1.0 + 0.001 * w) for w in range(W)])
    sel = rng.random(W) < 0.66
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    a.window_init(W, N, d, 1, theta)
    b.window_init(W, N, d, 1, theta)
    a.window_push(X[:, :T], y[:, :T])
    b.window_push(X[::-1, :T], y[::-1, :T])
    la, ia = a.window_set_theta(new)
    lb, ib = b.window_set_theta(new[::-1], select=sel[::-1])
    assert np.all(ia == 0) and np.all(ib == 0)
    assert np.array_equal(la[sel], lb[::-1][sel])
    na, ga = a.window_nll_grad()
    nb, gb = b.window_nll_grad()
    assert np.array_equal(na[sel], nb[::-1][sel]) and np.array_equal(ga[sel], gb[::-1][sel])
    Xs = X[:, T - 10:T] + 0.05
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs[::-1])
    assert np.array_equal(ma[sel], mb[::-1][sel]) and np.array_equal(va[sel], vb[::-1][sel])
    oa, ob = a.window_push(X[:, T:], y[:, T:]), b.window_push(X[::-1, T:], y[::-1, T:])
    for u, v in zip(oa, ob):
        assert np.array_equal(u[sel], v[::-1][sel])
    for w in (0, 299, 599):
        assert abs(la[w] - window_logml(1, new[w], N, X[w], y[w], T)) <= TOL * abs(la[w])


def test_a_failed_window_is_revived_by_set_theta(engine):
    """Window 1 of three fails at its first tick (sigma_n^2 < -sigma_f^2: a negative first pivot, a numerical status); the pushes
    go on past N so the ring moves; its forecasts are NaN.  set_theta with a valid theta for that window alone brings it back:
    info 0, forecasts and later pushes in parity with the oracle; the other two are bitwise what they are without the call."""
    W, N, d, T, K, M = 3, 24, 1, 70, 8, 30
    Xw, yw = zip(*[stream(T + K, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    theta[1, -1] = -2.0 * theta[1, 0]
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 0, theta)
        with pytest.raises(engine.CgpError):
            c.window_push(X[:, :T], y[:, :T])
        assert c.window_state(1)[1] > 0 and c.window_state(1)[0] == N
    Xs = X[:, T - 1:T, :] + np.random.default_rng(2).random((W, M, 1)) * 5.0
    mean, var, rc = a.window_predict(Xs, check=False)
    assert rc > 0 and np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    nll, g = a.window_nll_grad()
    assert np.isnan(nll[1]) and np.all(np.isnan(g[1])) and np.all(np.isfinite(nll[[0, 2]])) and np.all(np.isfinite(g[[0, 2]]))
    good = theta_of(0, d) * np.array([1.5, 0.8, 2.0])
    new = np.tile(good, (W, 1))
    logml, info = a.window_set_theta(new, select=[0, 1, 0])
    assert np.all(info == 0) and a.window_state(1) == (N, 0)
    assert abs(logml[1] - window_logml(0, good, N, X[1], y[1], T)) <= TOL * abs(logml[1])
    ma, va = a.window_predict(Xs)
    close(ma[1], va[1], *sliding_window_forecast(0, good, N, X[1, :T], y[1, :T], Xs[1]))
    mb, vb, _ = b.window_predict(Xs, check=False)
    oa = a.window_push(X[:, T:], y[:, T:])
    check_ticks([o[1] for o in oa], stream_ticks(0, good, N, X[1], y[1], T, T + K))
    with pytest.raises(engine.CgpError):
        b.window_push(X[:, T:], y[:, T:])
    for w in (0, 2):
        assert np.array_equal(ma[w], mb[w]) and np.array_equal(va[w], vb[w])


def test_a_bad_theta_fails_a_healthy_window_and_a_second_call_brings_it_back(engine):
    W, N, d, T, K = 3, 24, 1, 40, 5
    Xw, yw = zip(*[stream(T + K, d, 700 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 0, theta)
        c.window_push(X[:, :T], y[:, :T])
    bad = theta.copy()
    bad[2, -1] = -2.0 * bad[2, 0]
    logml, info, rc = a.window_set_theta(bad, select=[0, 0, 1], check=False)
    assert rc == 3 and list(info) == [0, 0, 1] and np.isnan(logml[2])
    with pytest.raises(engine.CgpError):
        a.window_set_theta(bad, select=[0, 0, 1])
    assert a.window_state(2) == (N, 1) and a.window_state(0) == (N, 0)
    Xs = X[:, T - 5:T] + 0.5
    mean, var, code = a.window_predict(Xs, check=False)
    assert code == 1 and np.all(np.isnan(mean[2]))
    mb, vb = b.window_predict(Xs)
    assert np.array_equal(mean[:2], mb[:2]) and np.array_equal(var[:2], vb[:2])
    # a NaN theta is a failed window too, not an argument error
    nan = theta.copy()
    nan[2, 1] = np.nan
    assert a.window_set_theta(nan, select=[0, 0, 1], check=False)[2] == 3
    logml, info = a.window_set_theta(theta, select=[0, 0, 1])
    assert info[2] == 0 and a.window_state(2) == (N, 0)
    oa, ob = a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])
    for u, v in zip(oa, ob):
        assert np.array_equal(u[:2], v[:2])
        assert np.max(np.abs(u[2] - v[2]) / np.maximum(np.abs(v[2]), 1e-3)) < 1e-9


def test_empty_windows_take_a_theta(engine):
    N, d = 20, 1
    X, y = stream(30, d, 3)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(2, N, d, 2, theta_of(2, d))
    new = other_theta(2, d)
    logml, info = ctx.window_set_theta(new)
    assert np.all(logml == 0.0) and np.all(info == 0) and ctx.window_state(0) == (0, 0)
    nll, g = ctx.window_nll_grad()
    assert np.all(nll == 0.0) and np.all(g == 0.0)
    out = ctx.window_push(np.stack([X, X]), np.stack([y, y]))
    check_ticks([o[1] for o in out], go.sliding_window_stream(2, new, N, X, y))


# ---- cgp_window_nll_grad -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,N,d", [(2, 40, 1), (0, 33, 2), (1, 64, 3), (1, 100, 6)])
def test_nll_grad_matches_the_oracle_along_a_stream(engine, kid, N, d):
    """Value and gradient from the resident factor (no refit) while filling, full, either side of a compaction and after the
    window has turned over; against the oracle and against cgp_nll_grad on a host copy of the same samples."""
    T = 3 * N + 6
    X, y = stream(T, d, 500 + N)
    theta = theta_of(kid, d)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta)
    batch = engine.Context(max_n=N, max_m=N, max_d=d)
    fed = 0
    for t in (1, 5, N // 2, N - 1, N, 2 * N - 1, 2 * N, 2 * N + 1, T):
        ctx.window_push(X[fed:t][None], y[fed:t][None])
        fed = t
        nll, g = ctx.window_nll_grad()
        onll, og = window_nll_grad(kid, theta, N, X, y, t)
        assert abs(nll[0] - onll) <= TOL * max(abs(onll), 1.0), (t, nll, onll)
        assert np.max(np.abs(g[0] - og)) <= TOL * np.max(np.abs(og)), (t, g, og)
        if t >= 2:
            Xw, yw = window_of(N, X, y, t)
            bn, bg = batch.nll_grad(Xw, yw, kid, theta)
            assert abs(nll[0] - bn) <= TOL * max(abs(bn), 1.0) and np.max(np.abs(g[0] - bg)) <= TOL * np.max(np.abs(bg))


def test_nll_grad_is_the_derivative_of_set_thetas_value(engine):
    """Central finite differences of -logML through cgp_window_set_theta on one window: no oracle involved."""
    N, d, T = 64, 3, 150
    X, y = stream(T, d, 21)
    theta = other_theta(1, d)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta_of(1, d))
    ctx.window_push(X[None], y[None])
    ctx.window_set_theta(theta)
    _, g = ctx.window_nll_grad()
    for i in range(len(theta)):
        h = 1e-5 * theta[i]
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = -(ctx.window_set_theta(tp)[0][0] - ctx.window_set_theta(tm)[0][0]) / (2 * h)
        assert abs(fd - g[0, i]) <= 1e-4 * max(abs(g[0, i]), 1e-3 * np.max(np.abs(g[0]))), (i, fd, g[0, i])


def test_nll_grad_is_read_only_and_host_form_is_device_form(engine):
    """push A, nll_grad, push B = push A, push B on a second context, bitwise; the device form on the caller's stream writes
    the same bits as the host form."""
    import torch
    W, N, d, T, K = 3, 48, 2, 170, 30
    Xw, yw = zip(*[stream(T + K, d, 60 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.stack([other_theta(1, d, w) for w in range(W)])
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 1, theta)
        c.window_push(X[:, :T], y[:, :T])
    nll, g = a.window_nll_grad()
    dn = torch.full((W,), -1.0, dtype=torch.float64, device="cuda")
    dg = torch.full((W, 6), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert a.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), 6, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), nll) and np.array_equal(dg.cpu().numpy()[:, :4], g)
    assert np.all(dg.cpu().numpy()[:, 4:] == -1.0)
    Xs = X[:, T - 9:T] + 0.2
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs)
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    for u, v in zip(a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])):
        assert np.array_equal(u, v)
    # set_theta: device form = host form
    new = np.stack([other_theta(1, d, 3 + w) for w in range(W)])
    dth = torch.from_numpy(np.pad(new, ((0, 0), (0, 2)))).cuda()
    dsel = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    dl = torch.full((W,), -1.0, dtype=torch.float64, device="cuda")
    di = torch.full((W,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert a.window_set_theta_device(dth.data_ptr(), 6, dsel.data_ptr(), dl.data_ptr(), di.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    hl, hi = b.window_set_theta(new, select=[1, 0, 1])
    assert np.array_equal(dl.cpu().numpy()[[0, 2]], hl[[0, 2]]) and dl.cpu().numpy()[1] == -1.0
    assert list(di.cpu().numpy()) == [0, -1, 0]
    for u, v in zip(a.window_nll_grad(), b.window_nll_grad()):
        assert np.array_equal(u, v)


def test_device_forms_replay_from_a_hip_graph(engine):
    """set_theta_device + nll_grad_device captured into a graph on a side stream and replayed with new thetas in the same
    device buffer: every replay's value and gradient are the oracle's at that theta."""
    import torch
    N, d, T = 40, 2, 100
    X, y = stream(T, d, 17)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta_of(1, d))
    ctx.window_push(X[None], y[None])
    ctx.synchronize()
    dth = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    dl = torch.zeros(1, dtype=torch.float64, device="cuda")
    di = torch.zeros(1, dtype=torch.int32, device="cuda")
    dn = torch.zeros(1, dtype=torch.float64, device="cuda")
    dg = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    dth.copy_(torch.from_numpy(other_theta(1, d)[None]))
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        assert ctx.window_set_theta_device(dth.data_ptr(), 4, 0, dl.data_ptr(), di.data_ptr(), s) == 0
        assert ctx.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), 4, s) == 0
    for k in range(3):
        theta = other_theta(1, d, k)
        dth.copy_(torch.from_numpy(theta[None]))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        onll, og = window_nll_grad(1, theta, N, X, y, T)
        assert di.item() == 0 and abs(dl.item() + onll) <= TOL * abs(onll)
        assert abs(dn.item() - onll) <= TOL * abs(onll) and np.max(np.abs(dg.cpu().numpy()[0] - og)) <= TOL * np.max(np.abs(og))


# ---- cgp_window_optimize -------------------------------------------------------------------------------------------------
def test_window_optimize_matches_optimize_batch_on_the_same_samples(engine):
    """Same optimiser, same start, same samples: final theta and logML agree with cgp_optimize_batch (the bars of
    test_gpu_optimize.py); logML is not below the start; unselected windows are untouched; pushes and a forecast afterwards
    are in parity under the returned theta."""
    W, N, d, T, K = 3, 192, 3, 260, 5
    Xw, yw = zip(*[stream(T + K, d, 80 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta0 = np.tile(np.array([0.05, 1.0, 1.0, 1.0, 0.01]), (W, 1))
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 1, theta0)
        start = c.window_push(X[:, :T], y[:, :T])[2][:, -1]
    sel = np.array([1, 0, 1], dtype=bool)
    th, lml, nev = a.window_optimize(max_evals=200, select=sel)
    assert np.all(np.isnan(th[1])) and nev[1] == 0 and np.all(nev[sel] > 1) and np.all(nev[sel] <= 200)
    assert np.all(th[sel] > 0) and np.all(lml[sel] >= start[sel] - 1e-9)
    bctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
    bth, blml, bnev = bctx.optimize_batch(X[:, T - N:T], y[:, T - N:T], 1, theta0, max_evals=200)
    for w in (0, 2):
        # the value reported is the true logML at the returned theta, and the window holds that theta's factor
        assert lml[w] == pytest.approx(window_logml(1, th[w], N, X[w], y[w], T), rel=1e-8)
        assert lml[w] == pytest.approx(blml[w], rel=1e-6, abs=1e-4)
        np.testing.assert_allclose(th[w], bth[w], rtol=2e-3)
        assert abs(int(nev[w]) - int(bnev[w])) <= 3
    nll, _ = a.window_nll_grad()
    assert np.max(np.abs(nll[sel] + lml[sel]) / np.abs(lml[sel])) < 1e-9
    Xs = X[:, T - 20:T] + 0.1
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs)
    oa, ob = a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])
    assert np.array_equal(ma[1], mb[1]) and np.array_equal(va[1], vb[1])
    for u, v in zip(oa, ob):
        assert np.array_equal(u[1], v[1])
    for w in (0, 2):
        close(ma[w], va[w], *sliding_window_forecast(1, th[w], N, X[w, :T], y[w, :T], Xs[w]))
        check_ticks([o[w] for o in oa], stream_ticks(1, th[w], N, X[w], y[w], T, T + K))


def test_window_optimize_on_the_reference_window(engine):
    """The 134 training samples of the reference's 149-tick window streamed into a window of N = 134 (RBF x Brownian), optimised
    in place from the fixture's theta0: theta and logML at slipval_window_opt.npz's bars."""
    g = load_golden("slipval_window_opt")
    _, _, xtr, ytr = go.slip_node_split(g["time_array"], g["slip_array"])
    n = len(xtr)
    assert n == 134
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    ctx.window_init(1, n, 1, 2, g["theta0"])
    ctx.window_push(xtr[None], ytr[None, :, 0])
    th, lml, nev = ctx.window_optimize()
    assert nev[0] <= 1000 and np.all(th[0] > 0)
    assert lml[0] == pytest.approx(-go.nll_and_grad(2, th[0], xtr, ytr[:, 0])[0], rel=1e-8)
    assert abs(int(nev[0]) - int(g["n_evals"])) <= 2
    np.testing.assert_allclose(th[0], g["theta"], rtol=1e-4)
    assert lml[0] == pytest.approx(float(g["logml"]), rel=1e-6)


def test_window_optimize_rejects_a_non_positive_start_before_changing_anything(engine):
    N, d, T = 24, 1, 30
    X, y = stream(T + 3, d, 4)
    theta = np.tile(theta_of(0, d), (2, 1))
    theta[1, -1] = -2.0 * theta[1, 0]
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(2, N, d, 0, theta)
        with pytest.raises(engine.CgpError):
            c.window_push(np.stack([X[:T], X[:T]]), np.stack([y[:T], y[:T]]))
    with pytest.raises(engine.CgpError) as e:
        a.window_optimize()
    assert e.value.code == EINVAL
    th, lml, nev = a.window_optimize(select=[1, 0], max_evals=3)   # the healthy window alone is fine
    assert np.all(th[0] > 0) and 1 <= nev[0] <= 3


# ---- argument and state errors, symbols ----------------------------------------------------------------------------------
def test_error_paths_and_symbols(engine):
    lib = engine.load()
    for name in ("cgp_window_set_theta", "cgp_window_set_theta_device", "cgp_window_nll_grad", "cgp_window_nll_grad_device",
                 "cgp_window_optimize"):
        assert hasattr(ctypes.CDLL(engine.LIB_PATH), name) and name in engine.EXPORTS
    assert lib.cgp_abi_version() == 3
    ctx = engine.Context(max_n=8, max_m=8, max_d=2)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    buf, ibuf = np.zeros(16), np.zeros(4, dtype=np.int32)
    P, IP = buf.ctypes.data_as(dp), ibuf.ctypes.data_as(ip)
    assert lib.cgp_window_set_theta(ctx.h, P, 4, None, P, IP) == ESTATE
    assert lib.cgp_window_set_theta_device(ctx.h, 1, 4, None, None, None, None) == ESTATE
    assert lib.cgp_window_nll_grad(ctx.h, P, P, 4) == ESTATE
    assert lib.cgp_window_nll_grad_device(ctx.h, 1, 1, 4, None) == ESTATE
    assert lib.cgp_window_optimize(ctx.h, 10, None, P, 4, P, IP) == ESTATE
    ctx.window_init(1, 8, 2, 1, theta_of(1, 2))
    assert lib.cgp_window_set_theta(ctx.h, None, 4, None, P, IP) == EINVAL
    assert lib.cgp_window_set_theta(ctx.h, P, 3, None, P, IP) == EINVAL
    assert lib.cgp_window_set_theta_device(ctx.h, None, 4, None, None, None, None) == EINVAL
    assert lib.cgp_window_set_theta_device(ctx.h, 1, 3, None, None, None, None) == EINVAL
    assert lib.cgp_window_nll_grad(ctx.h, None, P, 4) == EINVAL and lib.cgp_window_nll_grad(ctx.h, P, None, 4) == EINVAL
    assert lib.cgp_window_nll_grad(ctx.h, P, P, 3) == EINVAL
    assert lib.cgp_window_nll_grad_device(ctx.h, None, 1, 4, None) == EINVAL
    assert lib.cgp_window_nll_grad_device(ctx.h, 1, 1, 3, None) == EINVAL
    assert lib.cgp_window_optimize(ctx.h, 10, None, P, 3, P, IP) == EINVAL
    # NULL logml / info / outputs are allowed
    th = theta_of(1, 2)
    assert lib.cgp_window_set_theta(ctx.h, th.ctypes.data_as(dp), 4, None, None, None) == 0
    assert lib.cgp_window_optimize(ctx.h, 5, None, None, 0, None, None) == 0
