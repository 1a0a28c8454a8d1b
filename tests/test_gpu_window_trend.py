"""GPU tests of the explicit-basis (trend) forecast from the resident windows (cgp_window_trend_reserve,
cgp_window_predict_trend[_device]): the last q of the P pushed columns are the basis at the samples.  Parity against
tests/trend_oracle.py refitted on the stream's last N samples at 1e-6 (multi_oracle.errors' metric extended to beta); routes and
slots bitwise.  Every compared window meets the oracle's own conditions (no jitter, cond(A) <= 1e6, pivots pass the rank rule by
1e3): asserted.  Basis: [1, u, u^2][:q], u = (x0 - c) / s with c, s the stream's mean and spread over its 2N + 8 ticks."""
import numpy as np
import pytest

import trend_oracle as to
import window_multi_oracle as wm
import test_gpu_window_paths as paths

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_window_trend.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def new_ctx(engine, W, N, d, kid, theta, P, q, max_m=40):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    ctx.window_multi_reserve(P)
    if q:
        assert ctx.window_trend_reserve(q, max_m) == 0
    return ctx


def streams(W, T, d, Pt, q, seed):
    """X (W, T, d), the pushed columns [targets + an offset and a drift | basis] (W, T, Pt + q), and the basis' (c, s) per stream."""
    Xw, Yw = zip(*[wm.stream(T, d, Pt, seed + 17 * w) for w in range(W)])
    X, Y = np.stack(Xw), np.stack(Yw)
    cs = [(float(X[w, :, 0].mean()), float(X[w, :, 0].std())) for w in range(W)]
    H = np.stack([to.basis(X[w, :, 0], *cs[w], q).T for w in range(W)])                       # (W, T, q)
    Y = Y + 0.1 + 0.05 * H[:, :, min(1, q - 1):min(1, q - 1) + 1] * np.arange(1, Pt + 1)[None, None, :]
    return X, np.concatenate([Y, H], axis=2), cs


def basis_at(Xs, cs, q):
    return np.stack([to.basis(Xs[w, :, 0], *cs[w], q) for w in range(len(Xs))])               # (W, q, M)


def close(out, w, kid, theta, N, X, Yfull, Xs, Hs, q, noise=True, what=""):
    """Window w of out = (mean, var, beta, logml, tinfo) against the refit of the stream's last N samples."""
    Pt = Yfull.shape[1] - q
    o = to.fit_predict_trend(kid, theta, X[-N:], Yfull[-N:, :Pt].T, Yfull[-N:, Pt:].T, Xs, Hs, noise)
    assert to.conditions_hold(o), (what, o.tinfo, o.jitter, o.cond, o.margin)
    mean, var, beta, logml, tinfo = (a[w] for a in out[:5])
    assert tinfo == 0, what
    e = to.errors(mean, var, beta, logml, o)
    for k, v in zip(("mean", "var", "beta", "logml"), e):
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    print(f"{what} cond(A) {o.cond:.3g} errors / bar: mean {e[0] / TOL:.3g} var {e[1] / TOL:.3g} beta {e[2] / TOL:.3g} logml {e[3] / TOL:.3g}")
    assert max(e) <= TOL, (what, e)


PARITY = [(2, 16, 1), (2, 17, 1), (1, 33, 2), (3, 40, 2), (4, 64, 3)]


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("Pt", [1, 3])
@pytest.mark.parametrize("kid,N,d", PARITY)
def test_forecast_matches_the_refit_oracle(engine, kid, N, d, Pt, q):
    """Three windows fed uneven pushes (1, 2, 5, 37, 3, 11, ... ticks) and forecast from at N, 2N - 1, 2N, 2N + 1 (both sides of the
    ring's compaction) and 2N + 8 ticks, M = 17 and 1 test points; var - the multi-target call's var is not negative."""
    W, T, P = 3, 2 * N + 8, Pt + q
    X, Y, cs = streams(W, T, d, Pt, q, 1000 * kid + N)
    theta = wm.theta_of(kid, d)
    rng = np.random.default_rng(N + P)
    ctx = new_ctx(engine, W, N, d, kid, theta, P, q)
    look = {N, 2 * N - 1, 2 * N, 2 * N + 1, T}
    cuts, t = set(look), 0
    for s in [1, 2, 5, 37, 3, 11] * 40:
        t += s
        cuts.add(min(t, T))
    fed = 0
    for t in sorted(cuts):
        ctx.window_push_multi(X[:, fed:t], Y[:, fed:t])
        fed = t
        if t not in look:
            continue
        Xs = np.stack([wm.points_for(kid, X[w], t, N, 17, rng) for w in range(W)])
        noise = bool(t & 1)
        for M in (17, 1):
            Hs = basis_at(Xs[:, :M], cs, q)
            out = ctx.window_predict_trend(Xs[:, :M], Hs, include_noise=noise)
            assert out[0].shape == (W, Pt, M) and out[1].shape == (W, M) and out[2].shape == (W, Pt, q) and out[3].shape == (W, Pt)
            _, v0, _ = ctx.window_predict_multi(Xs[:, :M], include_noise=noise)
            assert np.all(out[1] >= v0)
            for w in range(W):
                if M == 17 or w == 0:
                    close(out, w, kid, theta, N, X[w, :t], Y[w, :t], Xs[w, :M], Hs[w], q, noise, what=f"t {t} M {M} w {w}")


def test_fewer_samples_than_basis_columns_answer_nan(engine):
    """n < q, the empty window included: A is rank-deficient, pivot n + 1 fails; every output NaN."""
    W, N, d, kid, Pt, q, M = 2, 16, 1, 2, 2, 3, 5
    X, Y, cs = streams(W, 2 * N + 8, d, Pt, q, 4)
    ctx = new_ctx(engine, W, N, d, kid, wm.theta_of(kid, d), Pt + q, q)
    Xs = X[:, 3:3 + M] + 0.5
    Hs = basis_at(Xs, cs, q)
    for n in range(q):
        if n:
            ctx.window_push_multi(X[:, n - 1:n], Y[:, n - 1:n])
        mean, var, beta, logml, tinfo = ctx.window_predict_trend(Xs, Hs)
        assert list(tinfo) == [n + 1] * W
        assert np.all(np.isnan(mean)) and np.all(np.isnan(var)) and np.all(np.isnan(beta)) and np.all(np.isnan(logml))
    ctx.window_push_multi(X[:, q - 1:q + 4], Y[:, q - 1:q + 4])
    out = ctx.window_predict_trend(Xs, Hs)
    assert not out[4].any() and np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))


def test_the_call_does_not_touch_the_windows(engine):
    """push A, trend forecasts, push B = push A, push B on a second context, bitwise."""
    W, N, d, kid, Pt, q, T = 2, 48, 2, 1, 2, 2, 170
    X, Y, cs = streams(W, T, d, Pt, q, 70)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -30:] + 0.1
    Hs = basis_at(Xs, cs, q)
    outs = []
    for between in (True, False):
        ctx = new_ctx(engine, W, N, d, kid, theta, Pt + q, q)
        ctx.window_push_multi(X[:, :90], Y[:, :90])
        if between:
            ctx.window_predict_trend(Xs, Hs)
            ctx.window_predict_trend(Xs[:, :3], Hs[:, :, :3], include_noise=False)
        o = ctx.window_push_multi(X[:, 90:], Y[:, 90:]) + ctx.window_predict(Xs) + ctx.window_predict_multi(Xs) + ctx.window_predict_trend(Xs, Hs)
        outs.append(o + (np.array([ctx.window_state(w) for w in range(W)]),))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_host_device_graph_and_slot_agree_bitwise(engine):
    import torch
    W, N, d, kid, T, M, Pt, q = 3, 40, 3, 1, 100, 37, 3, 2
    P = Pt + q
    X, Y, cs = streams(W, T, d, Pt, q, 500)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -M:] + 0.2
    Hs = basis_at(Xs, cs, q)
    ctx, lone = new_ctx(engine, W, N, d, kid, theta, P, q), new_ctx(engine, 1, N, d, kid, theta, P, q)   # lone: the last window, in slot 0
    for i in range(T):   # (tick by tick: the same push kernel in both contexts)
        ctx.window_push_multi(X[:, i:i + 1], Y[:, i:i + 1])
        lone.window_push_multi(X[2:, i:i + 1], Y[2:, i:i + 1])
    ref = ctx.window_predict_trend(Xs, Hs)
    for a, b in zip(ref, ctx.window_predict_trend(Xs, Hs)):
        assert np.array_equal(a, b)
    for w in range(W):
        close(ref, w, kid, theta, N, X[w], Y[w], Xs[w], Hs[w], q, what=f"window {w}")
    for a, b in zip(ref, lone.window_predict_trend(Xs[2:], Hs[2:])):
        assert np.array_equal(a[2], b[0])
    dxs, dhs = torch.from_numpy(Xs).cuda(), torch.from_numpy(Hs).cuda()
    out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((W, Pt, M), (W, M), (W, Pt, q), (W, Pt))]
    dt = torch.empty(W, dtype=torch.int32, device="cuda")

    def clear():
        for t in out:
            t.fill_(-1.0)
        dt.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        for t, r in zip(out + [dt], ref):
            assert np.array_equal(t.cpu().numpy(), r)

    def enqueue(s):
        assert ctx.window_predict_trend_device(M, P, q, dxs.data_ptr(), dhs.data_ptr(), True, *[t.data_ptr() for t in out], dt.data_ptr(),
                                               stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    clear()
    graph.replay()
    check()


def test_failed_window_answers_nan_and_is_revived(engine):
    """test_gpu_window_multi.py's failure recipe: the victim answers NaN with tinfo = 0, the neighbours are bitwise what they are
    beside a healthy one; after a reviving set_theta it meets the oracle with no further call."""
    kid, W, N, d, Pt, q, victim, pre, T, tl, K, M = 1, 3, 32, 2, 2, 2, 1, 41, 9, 4, 6, 11
    ts = pre + tl
    X, y, bad, good = paths.failing_streams(kid, W, d, pre + T + K, 31, victim, ts)
    rng = np.random.default_rng(8)
    cs = [(float(X[w, :, 0].mean()), float(X[w, :, 0].std())) for w in range(W)]
    H = np.stack([to.basis(X[w, :, 0], *cs[w], q).T for w in range(W)])
    Y = np.concatenate([np.stack([y + 0.1] + [y * (1.5 + p) + rng.normal(0, 0.02, y.shape) for p in range(1, Pt)], axis=2), H], axis=2)
    others = np.arange(W) != victim
    A, B = new_ctx(engine, W, N, d, kid, bad, Pt + q, q), new_ctx(engine, W, N, d, kid, good, Pt + q, q)
    for c in (A, B):
        c.window_push_multi(X[:, :pre], Y[:, :pre])
    A.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T], check=False)   # the victim fails at tick tl + 1 of this push
    B.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T])
    assert A.window_state(victim) == (N, tl + 1)
    Xs = X[:, pre + T - M:pre + T] + 0.25
    Hs = basis_at(Xs, cs, q)
    *oa, code = A.window_predict_trend(Xs, Hs, check=False)
    ob = B.window_predict_trend(Xs, Hs)
    assert code == tl + 1 and not oa[4].any()
    for a, b in zip(oa[:4], ob[:4]):
        assert np.all(np.isnan(a[victim])) and np.array_equal(a[others], b[others]) and not np.any(np.isnan(a[others]))
    A.window_push_multi(X[:, pre + T:], Y[:, pre + T:], check=False)
    _, info = A.window_set_theta(good, select=~others)
    assert np.all(info == 0) and A.window_state(victim) == (N, 0)
    Xs = X[:, -M:] + 0.25
    Hs = basis_at(Xs, cs, q)
    out = A.window_predict_trend(Xs, Hs)
    for w in range(W):
        close(out, w, kid, good[w], N, X[w], Y[w], Xs[w], Hs[w], q, what=f"revived, window {w}")


def test_status_codes(engine):
    buf = np.zeros(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    lib, h = ctx.lib, ctx.h

    def host(P=3, q=1, M=2, xs=p, hs=p, mean=p, var=p, hh=h):
        return lib.cgp_window_predict_trend(hh, M, P, q, xs, hs, 1, mean, var, p, p, ip)

    def dev(P=3, q=1, M=2, k=None, hh=h):
        args = [a] * 7
        if k is not None:
            args[k] = None
        return lib.cgp_window_predict_trend_device(hh, M, P, q, args[0], args[1], 1, *args[2:], None)

    assert lib.cgp_window_trend_reserve(h, 1, 4) == ESTATE and host() == ESTATE and dev() == ESTATE     # no windows
    theta = wm.theta_of(2, 1)
    ctx.window_init(1, 8, 1, 2, theta)
    assert lib.cgp_window_trend_reserve(h, 1, 4) == ESTATE and host() == ESTATE and dev() == ESTATE     # no multi-target reservation
    ctx.window_multi_reserve(3)
    assert host() == ESTATE and dev() == ESTATE                                                         # no trend reservation
    for q, mm in ((0, 4), (3, 4), (17, 4), (1, 0)):                                                     # 1 <= q < P, max_m >= 1
        assert lib.cgp_window_trend_reserve(h, q, mm) == EINVAL
    assert ctx.window_trend_reserve(1, 4) == 0
    assert host(P=2) == EINVAL and host(q=2) == EINVAL and host(M=0) == EINVAL and dev(P=2) == EINVAL and dev(q=2) == EINVAL
    assert dev(M=0) == EINVAL and host(M=5) == ECAPACITY and dev(M=5) == ECAPACITY
    assert host(xs=None) == EINVAL and host(hs=None) == EINVAL and host(mean=None) == EINVAL and host(var=None) == EINVAL
    for k in range(7):
        assert dev(k=k) == EINVAL
    # the context stays usable: 12 ticks, then a forecast against the oracle
    X, Y, cs = streams(1, 12, 1, 2, 1, 3)
    ctx.window_push_multi(X, Y)
    Xs = (X[0, -1:] + 1.0 + np.arange(4.0)[:, None])[None]
    Hs = basis_at(Xs, cs, 1)
    close(ctx.window_predict_trend(Xs, Hs), 0, 2, theta, 8, X[0], Y[0], Xs[0], Hs[0], 1)
    ctx.window_init(1, 8, 1, 2, theta)                                                                  # the reservations go with the windows
    assert host() == ESTATE
    ctx.window_multi_reserve(3)
    assert host() == ESTATE                                                                             # ... and the trend's with the multi-target one
    c32 = engine.Context(max_n=8, max_m=8, max_d=1, dtype=engine.F32)
    assert c32.lib.cgp_window_trend_reserve(c32.h, 1, 4) == EINVAL and host(hh=c32.h) == EINVAL and dev(hh=c32.h) == EINVAL
