"""GPU tests of the leave-one-out objective of the resident sliding windows (cgp_window_loo_grad_reserve,
cgp_window_loo_nll_grad[_device], cgp_window_optimize_loo) through the C ABI.  Oracle: tests/window_loo_grad_oracle.py (the refit
oracle of tests/loo_grad_oracle.py on the window's samples in window order) at the project's fp64 bar, 1e-6 -- nlpd against
max(|nlpd|, 1), the gradient against its largest entry; tests/test_oracle_window_loo_grad.py holds every compared window to the
condition that bar rests on.  Routes through the batch engine at 1e-9, the contracts of include/corenav_gp.h bitwise."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden, ROOT
from adapt_oracle import window_of, stream_ticks
from forecast_oracle import sliding_window_forecast
import loo_grad_oracle as lgo
import window_loo_grad_oracle as wo
from window_loo_grad_oracle import stream, theta_of

pytestmark = pytest.mark.gpu
TOL = 1e-6
ROUTE = 1e-9
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h
WORST = {"nlpd": 0.0, "grad": 0.0, "logml": 0.0}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def new_ctx(engine, W, N, d, kid, theta, dtype=0, reserve=True):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d, dtype=dtype)
    ctx.window_init(W, N, d, kid, theta)
    if reserve:
        assert ctx.window_loo_grad_reserve() == 0
    return ctx


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def close(out, w, kid, theta, Xw, yw, what=""):
    """Window w of out = (nlpd, grad, logml) against the oracle on the samples (Xw, yw)."""
    nlpd, g, logml = out
    if len(yw) == 0:
        assert nlpd[w] == 0.0 and logml[w] == 0.0 and not g[w].any()
        return
    f, og, olm, jit = lgo.nlpd_and_grad(kid, theta, Xw, yw)
    e = (abs(nlpd[w] - f) / max(abs(f), 1.0), rel(g[w], og), abs(logml[w] - olm) / max(abs(olm), 1.0))
    for k, v in zip(WORST, e):
        WORST[k] = max(WORST[k], v)
    print(f"{what} window {w} n {len(yw)}: errors / bar: nlpd {e[0] / TOL:.3g} grad {e[1] / TOL:.3g} logml {e[2] / TOL:.3g}")
    assert jit == 0.0
    assert e[0] <= TOL, (what, w, nlpd[w], f)
    assert e[1] <= TOL, (what, w, g[w], og)
    assert e[2] <= TOL, (what, w, logml[w], olm)


def same(u, v):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(u, v))


# ---- parity with the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,N,d", wo.RING_SHAPES)
def test_value_and_gradient_match_the_refit_oracle_over_the_rings_states(engine, kid, N, d):
    """Three windows in ONE context, evaluated after every tick of ring_ticks(N) with uneven pushes between them: filling at the
    16-row block edges, full, either side of the tick that moves the ring's origin, after the window has turned over.  n grows
    inside one reservation, so every state but the first runs on a scratch that an earlier, shorter state wrote; a twin context
    that is evaluated at the last state only gives the same bits.  At every state nlpd is bitwise -cgp_window_loo's sum and logml
    bitwise -cgp_window_nll_grad's nll."""
    X, y, theta = wo.ring_case(kid, N, d)
    a, b = new_ctx(engine, wo.RING_W, N, d, kid, theta), new_ctx(engine, wo.RING_W, N, d, kid, theta)
    fed = 0
    for t in wo.ring_ticks(N):
        for c in (a, b):
            c.window_push(X[:, fed:t], y[:, fed:t])
        fed = t
        out = a.window_loo_nll_grad()
        for w in range(wo.RING_W):
            close(out, w, kid, theta[w], *window_of(N, X[w], y[w], t), what=f"kid {kid} N {N} d {d} t {t}")
        assert np.array_equal(out[0], -a.window_loo()[3]) and np.array_equal(out[2], -a.window_nll_grad()[0])
    assert same(b.window_loo_nll_grad(), out)
    print("largest errors of the parity tests so far:", WORST)


@pytest.mark.parametrize("kid,d", wo.FIVE)
def test_five_windows(engine, kid, d):
    """5 windows of N = 40: windows x chunks (3) and windows x super-tile pairs (1) are no multiples of the 4 waves of a
    workgroup; while filling and after the window has slid."""
    X, y, theta = wo.five_case(kid, d)
    ctx = new_ctx(engine, 5, wo.FIVE_N, d, kid, theta)
    fed = 0
    for t in wo.FIVE_T:
        ctx.window_push(X[:, fed:t], y[:, fed:t])
        fed = t
        out = ctx.window_loo_nll_grad()
        for w in range(5):
            close(out, w, kid, theta[w], *window_of(wo.FIVE_N, X[w], y[w], t), what=f"five kid {kid} t {t}")


@pytest.mark.parametrize("N", [512, 700])
def test_the_long_windows(engine, N):
    """N = 512, d = 3 after 700 ticks (36 super-tile pairs, more than the 32 chunks); N = 700 after 1 500 ticks (above 512, where
    the refactor and the forecast change form; 66 pairs, the last super-tile 60 rows live)."""
    _, T, kid, theta, X, y = wo.big_case(N)
    ctx = new_ctx(engine, 1, N, 3, kid, theta)
    ctx.window_push(X[None], y[None])
    out = ctx.window_loo_nll_grad()
    close(out, 0, kid, theta, *window_of(N, X, y, T), what=f"N {N}")
    print("largest errors of the parity tests so far:", WORST)
    if N == 512:
        assert out[0][0] == pytest.approx(249.16, abs=5e-3)


@pytest.mark.parametrize("src,pin", [("mp_rbfbrownian_n134", "loo_grad_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_grad_mp_m32_n134"),
                                     ("matern_mp_m52_n134", "loo_grad_mp_m52_n134")])
def test_50_digit_pins(engine, src, pin):
    g, p = load_golden(src), load_golden(pin)
    kid, X, y, theta = int(g["kernel_id"]), np.asarray(g["X"], dtype=np.float64), np.asarray(g["y"], dtype=np.float64).reshape(-1), g["theta"]
    X = X.reshape(len(y), -1)
    ctx = new_ctx(engine, 1, len(y), X.shape[1], kid, theta)
    ctx.window_push(X[None], y[None])
    nlpd, grad, _ = ctx.window_loo_nll_grad()
    e = abs(nlpd[0] - float(p["nlpd"])) / max(abs(float(p["nlpd"])), 1.0), rel(grad[0], p["grad"])
    print(pin, "errors / bar:", e[0] / TOL, e[1] / TOL)
    assert len(y) == 134 and e[0] <= TOL and e[1] <= TOL


# ---- bitwise contracts ---------------------------------------------------------------------------------------------------------
def three_windows(engine, T=170, K=30):
    W, N, d = 3, 48, 2
    Xw, yw = zip(*[stream(T + K, d, 60 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(1, d), (W, 1)) * (1.0 + 0.1 * np.arange(W))[:, None]
    return W, N, d, X, y, theta


def test_host_device_graph_replay_and_two_calls_agree_bitwise(engine):
    """The device form on the legacy stream, on the context's and replayed from a graph captured on a side stream writes the host
    form's bits; gap columns of a wider gradient are kept; nlpd and grad do not depend on whether logml is passed."""
    import torch
    W, N, d, X, y, theta = three_windows(engine)
    a = new_ctx(engine, W, N, d, 1, theta)
    a.window_push(X[:, :170], y[:, :170])
    host = a.window_loo_nll_grad()
    assert same(a.window_loo_nll_grad(), host)
    nl, g, none = a.window_loo_nll_grad(want_logml=False)
    assert none is None and np.array_equal(nl, host[0]) and np.array_equal(g, host[1])
    nth, stride = 4, 6
    f = lambda *s: torch.full(s, -1.0, dtype=torch.float64, device="cuda")
    dn, dg, dl = f(W), f(W, stride), f(W)

    def clear():
        for t in (dn, dg, dl):
            t.fill_(-1.0)
        torch.cuda.synchronize()

    def check(logml=True):
        a.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dn.cpu().numpy(), host[0]) and np.array_equal(dg.cpu().numpy()[:, :nth], host[1])
        assert np.all(dg.cpu().numpy()[:, nth:] == -1.0)
        assert np.array_equal(dl.cpu().numpy(), host[2] if logml else np.full(W, -1.0))

    for s in (0, engine.STREAM_CTX):
        clear()
        assert a.window_loo_nll_grad_device(dn.data_ptr(), dg.data_ptr(), stride, dl.data_ptr(), stream=s) == 0
        check()
    clear()
    assert a.window_loo_nll_grad_device(dn.data_ptr(), dg.data_ptr(), stride, 0, stream=0) == 0
    check(logml=False)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert a.window_loo_nll_grad_device(dn.data_ptr(), dg.data_ptr(), stride, dl.data_ptr(),
                                            stream=torch.cuda.current_stream().cuda_stream) == 0
    for _ in range(2):
        clear()
        graph.replay()
        check()


def test_a_window_does_not_depend_on_its_slot_or_its_neighbours(engine):
    """Slot 0 of 1 = slot 4 of 5 among windows with other data and other thetas."""
    N, d, kid, T = wo.FIVE_N, 3, 1, wo.FIVE_T[-1]
    X, y, theta = wo.five_case(kid, d)
    five, one = new_ctx(engine, 5, N, d, kid, theta), new_ctx(engine, 1, N, d, kid, theta[4])
    five.window_push(X[:, :T], y[:, :T])
    one.window_push(X[4:5, :T], y[4:5, :T])
    o5, o1 = five.window_loo_nll_grad(), one.window_loo_nll_grad()
    assert all(np.array_equal(u[4], v[0]) for u, v in zip(o5, o1))
    close(o1, 0, kid, theta[4], *window_of(N, X[4], y[4], T), what="slot")


def test_fp32_contexts_answer_in_fp64(engine):
    N, d, T = 40, 2, 60
    X, y = stream(T, d, 3)
    theta = theta_of(1, d)
    outs = []
    for dtype in (0, 1):
        ctx = new_ctx(engine, 1, N, d, 1, theta, dtype=dtype)
        ctx.window_push(X[None], y[None])
        outs.append(ctx.window_loo_nll_grad())
    assert same(*outs)


def test_the_call_does_not_touch_the_windows(engine):
    """Against a twin context that never made the call: the next push's outputs, the state words, the forecast, the logML gradient
    and the leave-one-out values are bitwise the same."""
    W, N, d, X, y, theta = three_windows(engine)
    T = 170
    a, b = new_ctx(engine, W, N, d, 1, theta), new_ctx(engine, W, N, d, 1, theta, reserve=False)
    for c in (a, b):
        c.window_push(X[:, :T - 20], y[:, :T - 20])
    a.window_loo_nll_grad()   # once in the middle of the stream as well
    for c in (a, b):
        c.window_push(X[:, T - 20:T], y[:, T - 20:T])
    a.window_loo_nll_grad()
    Xs = X[:, T - 9:T] + 0.2
    assert same(a.window_predict(Xs), b.window_predict(Xs))
    assert same(a.window_nll_grad(), b.window_nll_grad())
    assert same(a.window_loo(), b.window_loo())
    a.window_loo_nll_grad()
    assert same(a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:]))
    assert all(a.window_state(w) == b.window_state(w) for w in range(W))
    assert same(a.window_loo(), b.window_loo())


# ---- routes ------------------------------------------------------------------------------------------------------------------
def test_route_the_batch_objective_on_the_downloaded_samples(engine):
    """Right after cgp_window_set_theta with the theta the windows have (a fresh factor: the incremental updates' own error is not
    in the comparison), against cgp_loo_nll_grad_batch on the same samples at 1e-9."""
    W, N, d, kid, T = 3, 64, 3, 1, 150
    Xw, yw = zip(*[stream(T, d, 90 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.stack([theta_of(kid, d) * (1.0 + 0.1 * w) for w in range(W)])
    ctx = new_ctx(engine, W, N, d, kid, theta)
    ctx.window_push(X, y)
    ctx.window_set_theta(theta)
    nlpd, g, logml = ctx.window_loo_nll_grad()
    b = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
    assert b.loo_grad_reserve(W) == 0
    rc, bn, bg, bl, info = b.loo_nll_grad_batch(np.ascontiguousarray(X[:, -N:]), np.ascontiguousarray(y[:, -N:]), theta, kid)
    assert rc == 0 and not info.any()
    e = (np.max(np.abs(nlpd - bn) / np.maximum(np.abs(bn), 1.0)), max(rel(g[w], bg[w]) for w in range(W)),
         np.max(np.abs(logml - bl) / np.maximum(np.abs(bl), 1.0)))
    print("route errors / bar:", [v / ROUTE for v in e])
    assert max(e) <= ROUTE


def test_gradient_is_the_derivative_of_set_theta_and_window_loo(engine):
    """Central differences of -lpd_sum through cgp_window_set_theta + cgp_window_loo on one window: no oracle involved."""
    N, d, T = 64, 3, 150
    X, y = stream(T, d, 21)
    theta = theta_of(1, d) * np.array([1.3, 0.9, 1.1, 1.2, 0.8])
    ctx = new_ctx(engine, 1, N, d, 1, theta_of(1, d))
    ctx.window_push(X[None], y[None])
    ctx.window_set_theta(theta)
    _, g, _ = ctx.window_loo_nll_grad()

    def value(th):
        ctx.window_set_theta(th)
        return -ctx.window_loo()[3][0]

    for i in range(len(theta)):
        h = 1e-5 * theta[i]
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = (value(tp) - value(tm)) / (2 * h)
        print(i, fd, g[0, i])
        assert abs(fd - g[0, i]) <= 1e-4 * max(abs(g[0, i]), 1e-3 * np.max(np.abs(g[0]))), (i, fd, g[0, i])


# ---- failure ------------------------------------------------------------------------------------------------------------------
def test_empty_failed_and_revived_windows(engine):
    """Before any push: 0, zeros, 0.  Window 1 of three fails at its first tick (sigma_n^2 = -2 sigma_f^2): NaN in all three; the
    other two are right, and bitwise what they are in a context without the failed window's theta; cgp_window_set_theta revives
    it and it is right again."""
    W, N, d, T = 3, 24, 1, 70
    Xw, yw = zip(*[stream(T, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    bad = theta.copy()
    bad[1, -1] = -2.0 * bad[1, 0]
    a, b = new_ctx(engine, W, N, d, 0, bad), new_ctx(engine, W, N, d, 0, theta)
    nlpd, g, logml = a.window_loo_nll_grad()
    assert np.array_equal(nlpd, np.zeros(W)) and np.array_equal(g, np.zeros((W, 3))) and np.array_equal(logml, np.zeros(W))
    with pytest.raises(engine.CgpError):
        a.window_push(X, y)
    b.window_push(X, y)
    assert a.window_state(1)[1] > 0
    oa, ob = a.window_loo_nll_grad(), b.window_loo_nll_grad()
    assert all(np.all(np.isnan(o[1])) for o in oa)
    for w in (0, 2):
        close(oa, w, 0, theta[w], *window_of(N, X[w], y[w], T), what="beside a failed window")
        assert all(np.array_equal(u[w], v[w]) for u, v in zip(oa, ob))
    a.window_set_theta(theta, select=[0, 1, 0])
    assert a.window_state(1) == (N, 0)
    oa = a.window_loo_nll_grad()
    for w in range(W):
        close(oa, w, 0, theta[w], *window_of(N, X[w], y[w], T), what="revived")
    assert all(np.array_equal(u[w], v[w]) for u, v in zip(oa, ob) for w in (0, 2))


# ---- optimiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,N,T,theta0,evals", wo.OPT_CASES)
def test_optimize_loo_matches_optimize_loo_batch_on_the_same_samples(engine, kid, N, T, theta0, evals):
    """Same optimiser, same start, same samples (the bars of test_window_optimize_matches_optimize_batch_on_the_same_samples);
    tests/test_oracle_window_loo_grad.py shows that no trial point of these cases needs the ladder the batch route has.  Afterwards
    the window holds the optimum's factor: the value is cgp_window_loo's, a forecast and four more pushes meet the refit oracle."""
    K = 4
    X, y = stream(T + K, 1, 7)
    theta0 = np.array(theta0)
    ctx = new_ctx(engine, 1, N, 1, kid, theta0)
    ctx.window_push(X[None, :T], y[None, :T])
    start = -ctx.window_loo_nll_grad()[0][0]
    th, lpd, nev = ctx.window_optimize_loo(max_evals=200)
    b = engine.Context(max_n=N, max_m=N, max_d=1, max_batch=1)
    assert b.loo_grad_reserve(1) == 0
    Xw, yw = window_of(N, X, y, T)
    bth, blpd, _, bnev = b.optimize_loo_batch(Xw[None], yw[None], kid, theta0, max_evals=200)
    print(kid, N, th[0], bth[0], lpd[0], blpd[0], nev[0], bnev[0], "scipy", evals)
    assert np.all(th[0] > 0) and 1 < nev[0] <= 200 and lpd[0] >= start - 1e-9
    assert lpd[0] == pytest.approx(blpd[0], rel=1e-6, abs=1e-4)
    np.testing.assert_allclose(th[0], bth[0], rtol=2e-3)
    assert abs(int(nev[0]) - int(bnev[0])) <= 3
    tot = ctx.window_loo()[3][0]
    assert abs(lpd[0] - tot) <= ROUTE * max(abs(tot), 1.0)
    assert lpd[0] == pytest.approx(-lgo.nlpd_and_grad(kid, th[0], Xw, yw)[0], rel=1e-8)
    Xs = X[T - 1, 0] + 1.0 + np.arange(5, dtype=np.float64)[:, None] if kid == 2 else X[T - 10:T] + 0.3
    mean, var = ctx.window_predict(Xs[None])
    omu, ovar = sliding_window_forecast(kid, th[0], N, X[:T], y[:T], Xs)
    assert np.max(np.abs(mean[0] - omu)) <= TOL * max(np.max(np.abs(omu)), 1e-12) and np.max(np.abs(var[0] - ovar) / ovar) < TOL
    pm, pv, lm = (o[0] for o in ctx.window_push(X[None, T:], y[None, T:]))
    om, ov, ol = stream_ticks(kid, th[0], N, X, y, T, T + K)
    assert np.max(np.abs(pm - om)) <= TOL * max(np.max(np.abs(om)), np.max(np.sqrt(ov)))
    assert np.max(np.abs(pv - ov) / ov) < TOL and np.max(np.abs(lm - ol) / np.maximum(np.abs(ol), 1.0)) < TOL


def test_optimize_loo_leaves_unselected_windows_alone_and_rejects_a_bad_start(engine):
    W, N, d, T = 3, 24, 1, 40
    Xw, yw = zip(*[stream(T + 3, d, 40 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(np.array([0.05, 1.0, 0.01]), (W, 1))
    a, b = new_ctx(engine, W, N, d, 0, theta), new_ctx(engine, W, N, d, 0, theta)
    for c in (a, b):
        c.window_push(X[:, :T], y[:, :T])
    th, lpd, nev = a.window_optimize_loo(max_evals=30, select=[1, 0, 1])
    assert np.all(np.isnan(th[1])) and np.isnan(lpd[1]) and nev[1] == 0 and np.all(nev[[0, 2]] > 1) and np.all(th[[0, 2]] > 0)
    oa, ob = a.window_loo_nll_grad(), b.window_loo_nll_grad()
    assert all(np.array_equal(u[1], v[1]) for u, v in zip(oa, ob))
    assert np.max(np.abs(oa[0][[0, 2]] + lpd[[0, 2]]) / np.maximum(np.abs(lpd[[0, 2]]), 1.0)) <= ROUTE
    pa, pb = a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])
    assert all(np.array_equal(u[1], v[1]) for u, v in zip(pa, pb))
    # a start theta <= 0 in a selected window: refused before anything changes
    bad = theta.copy()
    bad[1, -1] = -2.0 * bad[1, 0]
    c = new_ctx(engine, W, N, d, 0, bad)
    with pytest.raises(engine.CgpError):
        c.window_push(X[:, :T], y[:, :T])
    before = c.window_loo_nll_grad()
    with pytest.raises(engine.CgpError) as e:
        c.window_optimize_loo()
    assert e.value.code == EINVAL and same(c.window_loo_nll_grad(), before)
    th, _, nev = c.window_optimize_loo(select=[1, 0, 1], max_evals=3)
    assert np.all(th[[0, 2]] > 0) and np.all(nev[[0, 2]] >= 1) and np.all(nev[[0, 2]] <= 3)


# ---- status codes, symbols -----------------------------------------------------------------------------------------------------
def test_status_codes_and_symbols(engine):
    lib = engine.load()
    names = ("cgp_window_loo_grad_reserve", "cgp_window_loo_nll_grad", "cgp_window_loo_nll_grad_device", "cgp_window_optimize_loo")
    for name in names:
        assert hasattr(ctypes.CDLL(engine.LIB_PATH), name) and name in engine.EXPORTS
    assert lib.cgp_abi_version() == 3
    with open(os.path.join(ROOT, "include", "corenav_gp.h")) as fh:
        header = fh.read()
    assert all(f"int {name}(cgp_ctx *ctx" in header for name in names)
    ctx = engine.Context(max_n=8, max_m=8, max_d=2)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    buf, ibuf = np.zeros(16), np.zeros(4, dtype=np.int32)
    P, IP = buf.ctypes.data_as(dp), ibuf.ctypes.data_as(ip)
    assert lib.cgp_window_loo_grad_reserve(None) == ESTATE and lib.cgp_window_loo_nll_grad(None, P, P, 4, P) == ESTATE
    # no windows
    assert lib.cgp_window_loo_grad_reserve(ctx.h) == ESTATE
    assert lib.cgp_window_loo_nll_grad(ctx.h, P, P, 4, P) == ESTATE
    assert lib.cgp_window_loo_nll_grad_device(ctx.h, 1, 1, 4, None, None) == ESTATE
    assert lib.cgp_window_optimize_loo(ctx.h, 10, None, P, 4, P, IP) == ESTATE
    # windows, no reservation
    ctx.window_init(1, 8, 2, 1, theta_of(1, 2))
    assert lib.cgp_window_loo_nll_grad(ctx.h, P, P, 4, P) == ESTATE
    assert lib.cgp_window_loo_nll_grad_device(ctx.h, 1, 1, 4, None, None) == ESTATE
    assert lib.cgp_window_optimize_loo(ctx.h, 10, None, P, 4, P, IP) == ESTATE
    assert ctx.window_loo_grad_reserve() == 0 and ctx.window_loo_grad_reserve() == 0   # a second call replaces the first
    assert lib.cgp_window_loo_nll_grad(ctx.h, None, P, 4, P) == EINVAL and lib.cgp_window_loo_nll_grad(ctx.h, P, None, 4, P) == EINVAL
    assert lib.cgp_window_loo_nll_grad(ctx.h, P, P, 3, P) == EINVAL
    assert lib.cgp_window_loo_nll_grad_device(ctx.h, None, 1, 4, None, None) == EINVAL
    assert lib.cgp_window_loo_nll_grad_device(ctx.h, 1, None, 4, None, None) == EINVAL
    assert lib.cgp_window_loo_nll_grad_device(ctx.h, 1, 1, 3, None, None) == EINVAL
    assert lib.cgp_window_optimize_loo(ctx.h, 10, None, P, 3, P, IP) == EINVAL
    assert lib.cgp_window_loo_nll_grad(ctx.h, P, P, 4, None) == 0   # NULL logml is allowed
    # cgp_window_init drops the reservation
    ctx.window_init(1, 8, 2, 1, theta_of(1, 2))
    assert lib.cgp_window_loo_nll_grad(ctx.h, P, P, 4, P) == ESTATE
