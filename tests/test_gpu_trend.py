"""GPU parity of the explicit-basis (trend) fits (cgp_fit_predict_trend_batch[_device]: q basis columns ride through the multi-target
machinery, then the q x q normal equations, beta, the corrected mean / variance / evidence) against tests/trend_oracle.py, through
engine.py.  Bars are test_gpu_multi.py's: 1e-6 against the oracle in multi_oracle.errors' metric extended to beta (a column's beta
against that column's largest |beta|), 1e-9 between two schedules, bitwise wherever the header promises it.  Every input that is
compared with the oracle meets the oracle's own conditions (trend_oracle.conditions_hold: no jitter, cond(A) <= 1e6, every pivot
passes the rank rule by 1e3) -- asserted, so the bar cannot hide behind an ill-conditioned basis.  Shapes sit on the tile edges:
P + q across the 64- and 128-row tiles of the solve and the 16-column chunks of the Gram kernel, N across the 4-sample blocks."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import trend_oracle as to
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_trend.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def basis(x0, c, s, q):
    """[1, u, u^2][:q]; beyond three columns (the q = 16 tile-edge case) sines and cosines of u at rising frequency."""
    H = to.basis(x0, c, s, min(q, 3))
    u = (np.asarray(x0, dtype=np.float64) - c) / s
    wave = lambda r: (np.sin if r % 2 else np.cos)(1.7 * ((r - 1) // 2) * u)
    return np.concatenate([H] + [wave(r)[None] for r in range(3, q)]) if q > 3 else H


def window(N, d, P, seed, tick0=11):
    """test_gpu_multi.py::window with an offset and a drift per column: what a zero-mean model cannot forecast."""
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1)), t) + 0.1 + 0.0005 * (p % 5) * (t - t[0]) for p in range(P)])
    if d == 1:
        return t[:, None], Y
    return np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [rng.normal(size=N) for _ in range(d - 1)]), Y


def points_for(kid, X, M, rng):
    if kid == 2:
        return X[-1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    N = len(X)
    return X[rng.integers(max(0, N - 50), N, size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def problem(B, N, d, M, P, q, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, Yw = zip(*[window(N, d, P, seed + 17 * b, tick0=11 + b) for b in range(B)])
    X, Y = np.stack(Xw), np.stack(Yw)
    Xs = np.stack([points_for(kid, X[b], M, rng) for b in range(B)])
    cs = [(float(X[b, :, 0].mean()), float(max(X[b, :, 0].std(), 1e-3))) for b in range(B)]
    H = np.stack([basis(X[b, :, 0], *cs[b], q) for b in range(B)])
    Hs = np.stack([basis(Xs[b, :, 0], *cs[b], q) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return X, Y, H, Xs, Hs, theta, rng


def ctx_for(engine, B, N, d, M, P):
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    assert ctx.multi_reserve(B, P + 16) == 0 and ctx.trend_reserve(B, P, M) == 0
    return ctx


def close(kid, theta, X, Y, H, Xs, Hs, mean, var, beta, logml, noise=True, tol=TOL, need_conditions=True):
    o = to.fit_predict_trend(kid, theta, X, Y, H, Xs, Hs, noise)
    if need_conditions:
        assert to.conditions_hold(o), (o.tinfo, o.jitter, o.cond, o.margin)
    e = to.errors(mean, var, beta, logml, o)
    for k, v in zip(("mean", "var", "beta", "logml"), e):
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    print(f"cond(A) {o.cond:.3g}; errors / bar: mean {e[0] / tol:.3g} var {e[1] / tol:.3g} beta {e[2] / tol:.3g} logml {e[3] / tol:.3g}")
    assert max(e) <= tol, e
    assert np.all(var - o.base >= -1e-9 * o.base)   # the price of not knowing beta is not negative
    return o


@pytest.mark.parametrize("kid,d", [(0, 3), (1, 3), (2, 1), (3, 3), (4, 3)])
def test_every_kernel(engine, kid, d):
    B, N, M, P, q = 2, 130, 17, 3, 2
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, 10 * kid + d)
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    assert rc == 0 and not info.any() and not tinfo.any()
    assert mean.shape == (B, P, M) and var.shape == (B, M) and beta.shape == (B, P, q) and logml.shape == (B, P)
    for b in range(B):
        close(kid, theta[b], X[b], Y[b], H[b], Xs[b], Hs[b], mean[b], var[b], beta[b], logml[b])


@pytest.mark.parametrize("N,P,q,M", [(128, 1, 1, 64), (129, 63, 2, 1), (257, 127, 2, 65), (257, 120, 16, 17), (129, 14, 3, 64),
                                     (2, 1, 1, 1)])
def test_tile_edges(engine, N, P, q, M):
    B, d, kid = 2, 2, 1
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, N * P + M)
    ctx = ctx_for(engine, B, N, d, M, P)
    noise = bool((N + P) % 2)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid, include_noise=noise)
    assert rc == 0 and not info.any() and not tinfo.any()
    b = 1
    close(kid, theta[b], X[b], Y[b], H[b], Xs[b], Hs[b], mean[b], var[b], beta[b], logml[b], noise)


def test_first_term_of_var_is_the_multi_calls_var_and_the_multi_call_is_left_alone(engine):
    B, N, d, M, P, q, kid = 2, 257, 3, 65, 5, 3, 1
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, 5)
    ctx = ctx_for(engine, B, N, d, M, P)
    rc0, m0, v0, l0, _ = ctx.fit_predict_multi_batch(X, Y, Xs, theta, kid)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    rc1, m1, v1, l1, _ = ctx.fit_predict_multi_batch(X, Y, Xs, theta, kid)
    assert rc0 == 0 and rc == 0 and rc1 == 0 and not tinfo.any()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(l0, l1)
    for b in range(B):
        o = close(kid, theta[b], X[b], Y[b], H[b], Xs[b], Hs[b], mean[b], var[b], beta[b], logml[b])
        quad = o.var - o.base   # |L_A^-1 R|^2 in numpy: it involves neither Y nor beta
        assert np.all(var[b] >= v0[b]) and np.all(var[b] - v0[b] >= 0.0)
        gap = np.max(np.abs(var[b] - quad - v0[b]))
        print(f"fit {b}: max |var - quadratic form - multi var| = {gap:.3g} (bar 1e-12), largest quadratic form {quad.max():.3g}")
        assert gap <= 1e-12


def test_shifting_the_targets_by_the_basis_shifts_beta_and_the_mean(engine):
    B, N, d, M, P, q, kid = 2, 130, 2, 17, 3, 2, 1
    X, Y, H, Xs, Hs, theta, rng = problem(B, N, d, M, P, q, kid, 6)
    c = rng.normal(size=(B, P, q))
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, _, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    rc2, smean, svar, sbeta, slogml, _, stinfo = ctx.fit_predict_trend_batch(X, Y + c @ H, H, Xs, Hs, theta, kid)
    assert rc == 0 and rc2 == 0 and not tinfo.any() and not stinfo.any()
    eb = np.max(np.abs(sbeta - beta - c)) / max(1.0, np.max(np.abs(sbeta)))
    em = np.max(np.abs(smean - mean - c @ Hs)) / max(1.0, np.max(np.abs(smean)))
    el = np.max(np.abs(slogml - logml) / np.maximum(1.0, np.abs(logml)))
    print(f"shift: beta {eb:.3g} mean {em:.3g} logml {el:.3g} (bar 1e-9)")
    assert eb <= 1e-9 and em <= 1e-9 and el <= 1e-9 and np.array_equal(svar, var)


def test_one_sample_one_constant(engine):
    """N = 1, q = 1, H = Hs = 1: the constant is the sample -- mean = y, beta = y, logml = 0."""
    B, M, P = 2, 3, 2
    X = np.array([[[0.3]], [[-1.2]]])
    Y = np.array([[[0.7], [-0.2]], [[1.5], [0.1]]])
    Xs = np.tile(np.array([0.0, 0.4, 5.0])[None, :, None], (B, 1, 1))
    theta = np.tile(np.array([0.5, 1.0, 0.01]), (B, 1))
    ctx = ctx_for(engine, B, 1, 1, M, P)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, np.ones((B, 1, 1)), Xs, np.ones((B, 1, M)), theta, 0)
    assert rc == 0 and not info.any() and not tinfo.any()
    assert np.max(np.abs(mean - Y)) <= 1e-12 and np.max(np.abs(beta - Y)) <= 1e-12 and np.max(np.abs(logml)) <= 1e-12
    assert np.all(var > 0)


def test_column_permutation_and_p_independence_are_bitwise(engine):
    B, N, d, M, P, q, kid = 1, 257, 2, 65, 70, 2, 1
    X, Y, H, Xs, Hs, theta, rng = problem(B, N, d, M, P, q, kid, 7)
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, _, _ = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    assert rc == 0
    perm = rng.permutation(P)
    rc, pm, pv, pb, pl, _, _ = ctx.fit_predict_trend_batch(X, Y[:, perm], H, Xs, Hs, theta, kid)
    assert rc == 0 and np.array_equal(pm, mean[:, perm]) and np.array_equal(pb, beta[:, perm]) and np.array_equal(pl, logml[:, perm])
    assert np.array_equal(pv, var)
    rc, sm, sv, sb, sl, _, _ = ctx.fit_predict_trend_batch(X, Y[:, :3], H, Xs, Hs, theta, kid)   # the first 3 columns alone
    assert rc == 0 and np.array_equal(sm, mean[:, :3]) and np.array_equal(sb, beta[:, :3]) and np.array_equal(sl, logml[:, :3])
    assert np.array_equal(sv, var)


def test_slot_and_neighbour_independence_and_the_other_schedule(engine):
    """test_gpu_multi.py's shapes: a lone fit and a call of 3 take the same schedule (bitwise); a call of 40 takes another (1e-9)."""
    N, d, M, P, q, kid = 257, 2, 17, 5, 2, 1
    X, Y, H, Xs, Hs, theta, _ = problem(40, N, d, M, P, q, kid, 8)
    big = ctx_for(engine, 40, N, d, M, P)
    rc, bm, bv, bb, bl, _, bt = big.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    assert rc == 0 and not bt.any()
    three = ctx_for(engine, 3, N, d, M, P)
    sel = [4, 30, 17]
    rc, tm, tv, tb, tl, _, _ = three.fit_predict_trend_batch(X[sel], Y[sel], H[sel], Xs[sel], Hs[sel], theta[sel], kid)
    assert rc == 0
    one = ctx_for(engine, 1, N, d, M, P)
    for slot, b in enumerate(sel):
        rc, om, ov, ob, ol, _, _ = one.fit_predict_trend_batch(X[[b]], Y[[b]], H[[b]], Xs[[b]], Hs[[b]], theta[[b]], kid)
        assert rc == 0
        assert np.array_equal(om[0], tm[slot]) and np.array_equal(ov[0], tv[slot]) and np.array_equal(ob[0], tb[slot])
        assert np.array_equal(ol[0], tl[slot])
        assert np.max(np.abs(bm[b] - tm[slot])) <= 1e-9 * np.max(np.abs(tm[slot]))
        assert np.max(np.abs(bv[b] - tv[slot]) / tv[slot]) <= 1e-9
        assert np.max(np.abs(bb[b] - tb[slot])) <= 1e-9 * np.max(np.abs(tb[slot]))
        assert np.max(np.abs(bl[b] - tl[slot]) / np.maximum(1.0, np.abs(tl[slot]))) <= 1e-9
    close(kid, theta[30], X[30], Y[30], H[30], Xs[30], Hs[30], bm[30], bv[30], bb[30], bl[30])


def device_arrays(torch, X, Y, H, Xs, Hs, theta):
    B = X.shape[0]
    th = np.zeros((B, 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), Y, H, Xs.transpose(0, 2, 1), Hs, th)]


def device_outputs(torch, B, M, P, q, fill=0.0):
    f = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    i = lambda: torch.full((B,), -1, dtype=torch.int32, device="cuda")
    return f(B, P, M), f(B, M), f(B, P, q), f(B, P), i(), i()


def test_host_device_and_graph_replay_agree_bitwise(engine):
    import torch
    B, N, d, M, P, q, kid = 1, 257, 3, 53, 9, 3, 1
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, 10)
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, _, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    assert rc == 0 and not tinfo.any()
    dX, dY, dH, dXs, dHs, dth = device_arrays(torch, X, Y, H, Xs, Hs, theta)
    dm, dv, db, dl, di, dt = device_outputs(torch, B, M, P, q)

    def clear():
        for t in (dm, dv, db, dl):
            t.fill_(-1.0)
        di.fill_(-1)
        dt.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dv.cpu().numpy(), var)
        assert np.array_equal(db.cpu().numpy(), beta) and np.array_equal(dl.cpu().numpy(), logml)
        assert not di.cpu().numpy().any() and not dt.cpu().numpy().any()

    def enqueue(s):
        assert ctx.fit_predict_trend_batch_device(B, N, d, M, P, q, kid, dX.data_ptr(), dY.data_ptr(), dH.data_ptr(), dXs.data_ptr(),
                                                  dHs.data_ptr(), dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), db.data_ptr(),
                                                  dl.data_ptr(), di.data_ptr(), dt.data_ptr(), stream=s) == 0

    clear()
    enqueue(0)
    check()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    clear()
    graph.replay()
    check()


def test_jitter_ladder_is_per_fit(engine):
    """test_gpu_multi.py's ladder input: fit 1 needs the first rung and is re-submitted as a call of one fit; its trend is computed
    right after its retry, into its own slot.  Its means meet the oracle's jittered refit at 1e-5 (the bar the existing tests hold
    that near-singular fit to); fits 0 and 2 are bitwise what they are without the bad neighbour."""
    rng = np.random.default_rng(21)
    N, d, M, B, P, q = 200, 1, 7, 3, 3, 2
    X = np.stack([np.sort(rng.normal(size=(N, d)), 0) for _ in range(B)])
    Xgood = X.copy()
    X[1, :, 0] = np.repeat(np.arange(N // 2, dtype=float), 2)         # duplicated inputs -> rank deficient K
    cols = lambda x: np.stack([np.sin(x) + 0.4, np.cos(x) + 0.1 * x, np.sin(2.0 * x) + 0.5], axis=1)   # (B, P, N)
    Y, Ygood = cols(X[:, :, 0]), cols(Xgood[:, :, 0])
    Xs = np.tile(np.linspace(-1, 1, M)[None, :, None], (B, 1, 1))
    hb = lambda x: np.stack([to.basis(x[b, :, 0], float(x[b, :, 0].mean()), float(x[b, :, 0].std()), q) for b in range(B)])
    hs = lambda x: np.stack([to.basis(Xs[b, :, 0], float(x[b, :, 0].mean()), float(x[b, :, 0].std()), q) for b in range(B)])
    th = np.array([[1.0, 1.0, 0.05], [1.0, 3.0, -1e-8 - 2e-7], [1.0, 1.0, 0.05]])   # window 1: slightly indefinite
    thgood = np.array([[1.0, 1.0, 0.05]] * 3)
    assert go.fit(0, th[1], X[1], Y[1, 0]).jitter > 0
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, hb(X), Xs, hs(X), th, 0, include_noise=False)
    assert rc == 0 and not info.any() and not tinfo.any()
    o = to.fit_predict_trend(0, th[1], X[1], Y[1], hb(X)[1], Xs[1], hs(X)[1], False)
    em = np.max(np.max(np.abs(mean[1] - o.mean), axis=1) / np.max(np.abs(o.mean), axis=1))
    print(f"fit 1 (jitter {o.jitter:.3g}, cond(A) {o.cond:.3g}), mean error / 1e-5: {em / 1e-5:.3g}")
    assert o.jitter > 0 and em <= 1e-5 and np.all(np.isfinite(logml[1])) and np.all(np.isfinite(beta[1]))
    for b in (0, 2):
        close(0, th[b], X[b], Y[b], hb(X)[b], Xs[b], hs(X)[b], mean[b], var[b], beta[b], logml[b], False)
    rc, gm, gv, gb, gl, _, _ = ctx.fit_predict_trend_batch(Xgood, Ygood, hb(Xgood), Xs, hs(Xgood), thgood, 0, include_noise=False)
    assert rc == 0
    for b in (0, 2):
        assert np.array_equal(gm[b], mean[b]) and np.array_equal(gv[b], var[b]) and np.array_equal(gb[b], beta[b])
        assert np.array_equal(gl[b], logml[b])


def test_device_form_failed_fit_is_nan_with_tinfo_zero_neighbours_are_right(engine):
    import torch
    B, N, d, M, P, q, kid = 3, 200, 2, 30, 5, 2, 1
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, 9)
    theta[1, -1] = -2.0 * theta[1, 0]   # Ky of fit 1 is negative definite: no ladder in the device form
    ctx = ctx_for(engine, B, N, d, M, P)
    dX, dY, dH, dXs, dHs, dth = device_arrays(torch, X, Y, H, Xs, Hs, theta)
    dm, dv, db, dl, di, dt = device_outputs(torch, B, M, P, q)
    assert ctx.fit_predict_trend_batch_device(B, N, d, M, P, q, kid, dX.data_ptr(), dY.data_ptr(), dH.data_ptr(), dXs.data_ptr(),
                                              dHs.data_ptr(), dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), db.data_ptr(),
                                              dl.data_ptr(), di.data_ptr(), dt.data_ptr()) == 0
    torch.cuda.synchronize()
    info, tinfo, mean, var, beta, logml = (t.cpu().numpy() for t in (di, dt, dm, dv, db, dl))
    assert info[1] > 0 and info[0] == 0 and info[2] == 0 and not tinfo.any()
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(beta[1])) and np.all(np.isnan(logml[1]))
    for b in (0, 2):
        close(kid, theta[b], X[b], Y[b], H[b], Xs[b], Hs[b], mean[b], var[b], beta[b], logml[b])


@pytest.mark.parametrize("what", ["duplicate", "nan"])
def test_rank_rule(engine, what):
    """Fit 1's basis column 1 duplicates column 0 exactly, or holds a NaN: pivot 2 fails, tinfo = 2, NaN for that fit only."""
    B, N, d, M, P, q, kid = 3, 130, 2, 17, 3, 3, 1
    X, Y, H, Xs, Hs, theta, _ = problem(B, N, d, M, P, q, kid, 11)
    good = ctx_for(engine, B, N, d, M, P).fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, kid)
    Hbad = H.copy()
    if what == "duplicate":
        Hbad[1, 1] = Hbad[1, 0]
    else:
        Hbad[1, 1, 40] = np.nan
    ctx = ctx_for(engine, B, N, d, M, P)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, Hbad, Xs, Hs, theta, kid)
    assert rc == 0 and not info.any() and list(tinfo) == [0, 2, 0]
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(beta[1])) and np.all(np.isnan(logml[1]))
    for b in (0, 2):
        for a, g in zip((mean, var, beta, logml), good[1:5]):
            assert np.array_equal(a[b], g[b])
        close(kid, theta[b], X[b], Y[b], H[b], Xs[b], Hs[b], mean[b], var[b], beta[b], logml[b])


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.zeros(512)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 8, 1, 4, 2, 2, 2)   # batch, N, d, M, P, q, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, hh=p, xs=p, hs=p, th=p, stride=4, mean=p, var=p):
        return lib.cgp_fit_predict_trend_batch(h, *shape, x, y, hh, xs, hs, th, stride, 1, mean, var, p, p, ip, ip)

    def dev(h=ctx.h, shape=shape, y=a, hh=a, hs=a, mean=a, var=a, beta=a, logml=a, info=a, tinfo=a):
        return lib.cgp_fit_predict_trend_batch_device(h, *shape, a, y, hh, a, hs, a, None, 1, mean, var, beta, logml, info, tinfo, None)

    assert host() == ESTATE and dev() == ESTATE                                   # no reservation
    for f in (host, dev):                                                         # no context, M = 0, P = 0, q = 0, q = 17 come first
        assert f(h=None) == EINVAL
        for s in ((1, 8, 1, 0, 2, 2, 2), (1, 8, 1, 4, 0, 2, 2), (1, 8, 1, 4, 2, 0, 2), (1, 8, 1, 4, 2, 17, 2)):
            assert f(shape=s) == EINVAL
    assert lib.cgp_trend_reserve(None, 1, 2, 4) == EINVAL
    assert lib.cgp_trend_reserve(ctx.h, 1, 2, 4) == ESTATE                        # no multi-target reservation
    assert lib.cgp_multi_reserve(ctx.h, 1, 2 + 15) == 0
    assert lib.cgp_trend_reserve(ctx.h, 1, 2, 4) == ESTATE                        # ... one too small for P + 16
    assert lib.cgp_multi_reserve(ctx.h, 1, 2 + 16) == 0
    for mb, mp, mm in ((0, 2, 4), (3, 2, 4), (1, 0, 4), (1, 4097 - 16, 4), (1, 2, 0), (1, 2, 9)):
        assert lib.cgp_trend_reserve(ctx.h, mb, mp, mm) == EINVAL
    assert host() == ESTATE
    assert lib.cgp_trend_reserve(ctx.h, 1, 2, 4) == 0
    for s in ((1, 8, 1, 4, 3, 2, 2), (2, 8, 1, 4, 2, 2, 2), (1, 8, 1, 5, 2, 2, 2)):   # P, batch, M beyond the reservation
        assert host(shape=s) == ECAPACITY and dev(shape=s) == ECAPACITY
        assert host(shape=s, x=None) == ECAPACITY and dev(shape=s, y=None) == ECAPACITY   # ... before the arrays
    assert host(x=None) == EINVAL and host(y=None) == EINVAL and host(hh=None) == EINVAL and host(xs=None) == EINVAL
    assert host(hs=None) == EINVAL and host(th=None) == EINVAL and host(mean=None) == EINVAL and host(var=None) == EINVAL
    assert host(stride=3) == EINVAL
    for k in ("y", "hh", "hs", "mean", "var", "beta", "logml", "info", "tinfo"):
        assert dev(**{k: None}) == EINVAL, k
    assert host(shape=(1, 8, 1, 4, 2, 2, 5)) == EINVAL and host(shape=(1, 17, 1, 4, 2, 2, 2)) == ECAPACITY   # cgp_fit_predict_batch's own
    assert lib.cgp_multi_reserve(ctx.h, 1, 3) == 0                                # the multi-target reservation shrinks under it
    assert host() == ECAPACITY and dev() == ECAPACITY
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_trend_reserve(f32.h, 1, 2, 4) == EINVAL and host(h=f32.h) == EINVAL and dev(h=f32.h) == EINVAL
    # the context is still usable
    assert ctx.multi_reserve(2, 2 + 16) == 0 and ctx.trend_reserve(2, 2, 8) == 0
    X, Y, H, Xs, Hs, theta, _ = problem(2, 8, 1, 8, 2, 2, 2, 2)
    rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(X, Y, H, Xs, Hs, theta, 2)
    assert rc == 0 and not tinfo.any()
    close(2, theta[1], X[1], Y[1], H[1], Xs[1], Hs[1], mean[1], var[1], beta[1], logml[1])
