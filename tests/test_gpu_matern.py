"""GPU parity of the Matern 3/2 and 5/2 ARD kernels (CGP_KERNEL_MATERN32_ARD = 3, CGP_KERNEL_MATERN52_ARD = 4) through the C ABI:
single window, the three batch schedules, gradient and optimiser, the reference-shaped 134-sample window, the sliding windows
(push, forecast, joint covariance, sample paths, set_theta, gradient, optimiser), the refusals, and the squared-exponential /
Brownian results recorded before the kernels were added.  Reference values: tests/golden/matern_*.npz (scikit-learn, closed
forms, 50-digit mpmath: gen_matern_golden.py) and tests/matern_oracle.py, which test_oracle_matern.py pins to them.

`python tests/test_gpu_matern.py --record` writes the tests/golden/pre_matern_*.npy files from the library that is loaded."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):     # (run as a script, --record: the package and the test-support modules)
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import gp_oracle as go  # noqa: E402
import matern_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
GOLDEN = os.path.join(HERE, "golden")
KIDS = [mo.KERNEL_MATERN32_ARD, mo.KERNEL_MATERN52_ARD]
FIXTURES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "matern_*.npz")))


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def relv(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def window(seed, N, d, M, dense=False):
    rng = np.random.default_rng(seed)
    if d == 1 and dense:
        X = np.arange(7.0, 7.0 + N)[:, None]
        Xs = (7.0 + N + np.arange(float(M)))[:, None]
        theta = np.array([0.05, 25.0, 0.002])
    else:
        X = rng.uniform(-2.0, 2.0, (N, d))
        Xs = rng.uniform(-2.2, 2.2, (M, d))
        theta = np.concatenate([[0.9], rng.uniform(0.7, 2.5, d), [0.01]])
    y = np.sin(X @ rng.normal(size=d) / (10.0 if dense else 1.0)) + 0.05 * rng.normal(size=N)
    return X, y, Xs, theta


# ---- one window -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fit_predict_alpha_factor_match_fixture(engine, name):
    z = np.load(os.path.join(GOLDEN, name))
    kid, X, y, Xs, th = int(z["kernel_id"]), z["X"], z["y"], z["Xs"], z["theta"]
    N, d = X.shape
    ctx = engine.Context(max_n=N, max_m=max(len(Xs), N), max_d=d, max_batch=1)
    rc, logml = ctx.fit(X, y, kid, th)
    assert rc == 0 and ctx.last_jitter() == 0.0
    assert abs(logml - float(z["logml"])) <= TOL * abs(float(z["logml"]))
    mean, var = ctx.predict(Xs, include_noise=False)
    assert rel(mean, z["mean"]) < TOL and relv(var, z["var_latent"]) < TOL
    mean_n, var_n = ctx.predict(Xs, include_noise=True)
    assert np.array_equal(mean_n, mean) and relv(var_n, z["var_latent"] + th[-1]) < TOL
    assert rel(ctx.alpha(), z["alpha"]) < TOL
    if N <= 256:
        f = mo.fit(kid, th, X, y)
        L = ctx.factor()
        assert rel(L, f.L) < TOL and not np.any(np.triu(L, 1))
    nll, g = ctx.nll_grad(X, y, kid, th)
    assert abs(nll + float(z["logml"])) <= TOL * abs(float(z["logml"]))
    assert rel(-g, z["dlogml_dtheta"]) < TOL


@pytest.mark.parametrize("kid", KIDS)
@pytest.mark.parametrize("N,d,M", [(1, 1, 1), (2, 2, 3), (97, 1, 45), (203, 3, 131), (517, 6, 77), (1100, 2, 599)])
def test_ragged_shapes_match_oracle(engine, kid, N, d, M):
    X, y, Xs, th = window(N + d, N, d, M, dense=(d == 1))
    ctx = engine.Context(max_n=N, max_m=max(M, N), max_d=d, max_batch=1)
    rc, logml = ctx.fit(X, y, kid, th)
    f = mo.fit(kid, th, X, y)
    assert rc == 0 and ctx.last_jitter() == f.jitter
    mean, var = ctx.predict(Xs)
    omu, ovar = mo.predict(f, Xs)
    assert abs(logml - f.logml) <= TOL * max(abs(f.logml), 1.0)
    assert rel(mean, omu) < TOL and relv(var, ovar) < TOL and rel(ctx.alpha(), f.alpha) < TOL
    nll, g = ctx.nll_grad(X, y, kid, th)
    onll, og = mo.nll_and_grad(kid, th, X, y)
    assert abs(nll - onll) <= TOL * max(abs(onll), 1.0) and rel(g, og) < TOL


def test_coincident_points_give_the_amplitude(engine):
    """r = 0 off the diagonal: two identical inputs have covariance sigma_f^2, and the gradient stays finite."""
    for kid in KIDS:
        X = np.array([[0.3, 1.0], [0.3, 1.0], [0.9, -0.2]])
        y = np.array([0.2, 0.25, -0.4])
        th = np.array([1.1, 0.8, 1.9, 0.05])
        ctx = engine.Context(max_n=4, max_m=4, max_d=2, max_batch=1)
        rc, logml = ctx.fit(X, y, kid, th)
        f = mo.fit(kid, th, X, y)
        assert rc == 0 and abs(logml - f.logml) < TOL * abs(f.logml) and rel(ctx.factor(), f.L) < 1e-12
        nll, g = ctx.nll_grad(X, y, kid, th)
        assert np.all(np.isfinite(g)) and rel(g, mo.nll_and_grad(kid, th, X, y)[1]) < TOL


# ---- batch schedules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid", KIDS)
def test_batch_schedules_agree(engine, kid):
    """3, 40 and 200 fits (latency, mid-size, full-batch schedules): every fit equals the oracle to 1e-6 and the same fit in the
    three calls agrees to rounding (test_gpu_parity claims bitwise equality for repeated calls of ONE schedule only, which is
    what is claimed here too); a sweep repeated on one context is bitwise."""
    N, d, M, B = 300, 3, 70, 200
    W = [window(1000 + b, N, d, M) for b in range(B)]
    X, y, Xs, th = (np.stack([w[i] for w in W]) for i in range(4))
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    out = {}
    for nb in (3, 40, 200):
        rc, mean, var, logml, info = ctx.fit_predict_batch(X[:nb], y[:nb], Xs[:nb], th[:nb], kid)
        assert rc == 0 and not info.any()
        out[nb] = (mean, var, logml)
    rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th, kid)
    assert all(np.array_equal(a, b) for a, b in zip(out[200], (mean, var, logml)))
    for b in (0, 2, 39, 199):
        f = mo.fit(kid, th[b], X[b], y[b])
        omu, ovar = mo.predict(f, Xs[b])
        assert rel(out[200][0][b], omu) < TOL and relv(out[200][1][b], ovar) < TOL
        assert abs(out[200][2][b] - f.logml) < TOL * abs(f.logml)
    for nb in (3, 40):
        for a, b in zip(out[nb], out[200]):
            assert rel(a, b[:nb]) < 1e-10


# ---- gradient and optimiser -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kid", [("m32", 3), ("m52", 4)])
def test_optimize_reaches_scipy_optimum_on_slip_window(engine, tag, kid):
    z = np.load(os.path.join(GOLDEN, f"matern_mp_{tag}_n134.npz"))
    X, y = z["X"], z["y"]
    ctx = engine.Context(max_n=256, max_m=1024, max_d=1, max_batch=4)
    nll, g = ctx.nll_grad(X, y, kid, z["theta"])          # the 50-digit pin
    assert abs(nll + float(z["logml"])) < TOL * abs(float(z["logml"])) and rel(-g, z["dlogml_dtheta"]) < TOL
    oth, ologml, oev = mo.optimize(kid, X, y)
    th, logml, nev = ctx.optimize(X, y, kid, np.ones(3))
    assert abs(logml - ologml) <= TOL * abs(ologml)
    assert abs((nev - 1) - oev) <= 3                      # host optimiser: + 1 for the refit at the optimum (corenav_gp.h)
    mean, var = ctx.predict(z["Xs"])                      # the context is left fitted at the optimum
    omu, ovar = mo.predict(mo.fit(kid, th, X, y), z["Xs"])
    assert rel(mean, omu) < TOL and relv(var, ovar) < TOL
    # batch form = per-window form
    Xb = np.stack([X, X[::-1].copy(), X])
    yb = np.stack([y, y[::-1].copy(), 0.5 * y])
    thb, lb, nb = ctx.optimize_batch(Xb, yb, kid, np.ones(3))
    for b in range(3):
        t1, l1, n1 = ctx.optimize(Xb[b], yb[b], kid, np.ones(3))
        assert abs(l1 - lb[b]) <= TOL * abs(l1) and rel(thb[b], t1) < 1e-4


# ---- the reference's shape: 134 samples, d = 1, 599 test points -----------------------------------------------------------------
@pytest.mark.parametrize("tag,kid", [("m32", 3), ("m52", 4)])
def test_reference_shaped_window_every_route(engine, tag, kid):
    z = np.load(os.path.join(GOLDEN, f"matern_sk_{tag}_n134_d1.npz"))
    s = np.load(os.path.join(GOLDEN, "slipval_window_rbfbrownian.npz"))
    X, y, Xs, th = z["X"], z["y"], z["Xs"], z["theta"]
    ctx = engine.Context(max_n=256, max_m=1024, max_d=1, max_batch=256)
    want_mu, want_var = z["mean"], z["var_latent"] + th[-1]
    rc, mean, var, logml, info = ctx.fit_predict_batch(X[None], y[None], Xs[None], th[None], kid)
    assert rc == 0 and rel(mean[0], want_mu) < TOL and relv(var[0], want_var) < TOL
    assert abs(logml[0] - float(z["logml"])) < TOL * abs(float(z["logml"]))
    # 256 windows: the fixture in slots 0, 100 and 255 between scaled neighbours -- independent of slot and neighbours
    scale = np.linspace(0.5, 1.5, 256)
    scale[[0, 100, 255]] = 1.0
    rc, mb, vb, lb, info = ctx.fit_predict_batch(np.tile(X, (256, 1, 1)), y[None] * scale[:, None], np.tile(Xs, (256, 1, 1)),
                                                  np.tile(th, (256, 1)), kid)
    assert rc == 0 and not info.any()
    for b in (0, 100, 255):
        assert np.array_equal(mb[b], mb[0]) and np.array_equal(vb[b], vb[0]) and lb[b] == lb[0]
        assert rel(mb[b], want_mu) < TOL and relv(vb[b], want_var) < TOL
    assert rel(mb[7], want_mu * scale[7]) < TOL
    m2, s2 = ctx.slip_node_callback(s["time_array"], s["slip_array"], th, kernel_id=kid)
    assert m2.shape == (599,) and rel(m2, want_mu) < TOL and relv(s2, 2.0 * np.sqrt(want_var)) < TOL
    rc, l1 = ctx.fit(X, y, kid, th)
    m3, v3 = ctx.predict(Xs)
    assert rc == 0 and rel(m3, want_mu) < TOL and relv(v3, want_var) < TOL
    m4, s4, th4 = ctx.slip_node_callback_opt(s["time_array"], s["slip_array"], np.ones(3), kernel_id=kid)
    oth, ologml, _ = mo.optimize(kid, X, y)
    omu, ovar = mo.predict(mo.fit(kid, th4, X, y), Xs)
    assert m4.shape == (599,) and rel(m4, omu) < TOL and relv(s4, 2.0 * np.sqrt(ovar)) < TOL
    assert abs(mo.fit(kid, th4, X, y).logml - ologml) < TOL * abs(ologml)


def test_slip_node_passes_the_kernel_through(engine):
    """The node's one-line kernel choice: GpSlipNode(kernel_id=...) publishes the 599 values of that kernel."""
    from corenav_gp_amd import gp_slip_node as node
    s = np.load(os.path.join(GOLDEN, "slipval_window_rbfbrownian.npz"))
    z = np.load(os.path.join(GOLDEN, "matern_sk_m52_n134_d1.npz"))
    got = []
    n = node.GpSlipNode(theta=z["theta"], optimize=False, kernel_id=engine.KERNEL_MATERN52_ARD, publisher=got.append)
    out = n.callback(node.GP_Input(s["time_array"], s["slip_array"]))
    assert got == [out] and len(out.mean) == 599 and rel(out.mean, z["mean"]) < TOL
    assert relv(out.sigma, 2.0 * np.sqrt(z["var_latent"] + z["theta"][-1])) < TOL
    n2 = node.GpSlipNode(kernel_id=engine.KERNEL_MATERN32_ARD)                 # optimising node: GPy's all-ones start of that kernel
    assert n2.theta.shape == (3,) and len(n2.callback(node.GP_Input(s["time_array"], s["slip_array"])).mean) == 599
    assert n2.last_theta.shape == (3,) and np.all(n2.last_theta > 0)
    with pytest.raises(ValueError):
        node.GpSlipNode(optimize=False, kernel_id=engine.KERNEL_MATERN32_ARD)


# ---- sliding windows ------------------------------------------------------------------------------------------------------------
def stream(T, d, seed, nwin):
    rng = np.random.default_rng(seed)
    t = np.arange(11.0, 11.0 + T)
    xs = np.empty((nwin, T, d))
    xs[:, :, 0] = (t - t.mean()) / 40.0
    xs[:, :, 1:] = rng.normal(size=(nwin, T, d - 1))
    ys = np.sin(xs[:, :, 0] * rng.uniform(0.5, 2.0, (nwin, 1))) + 0.05 * rng.normal(size=(nwin, T))
    return xs, ys


def check_stream(engine, kid, nwin, N, d, T, cuts, check_windows, ticks, extra=0):
    xs_all, ys_all = stream(T + extra, d, 5 * N + kid, nwin)      # `extra` more ticks of the same stream for the caller
    xs, ys = xs_all[:, :T], ys_all[:, :T]
    rng = np.random.default_rng(N)
    theta = np.column_stack([rng.uniform(0.5, 1.5, nwin)] + [rng.uniform(0.6, 1.8, nwin) for _ in range(d)] + [np.full(nwin, 1e-3)])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, theta)
    parts = [ctx.window_push(xs[:, a:b], ys[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pm, pv, lm = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
    for w in check_windows:
        assert ctx.window_state(w) == (min(N, T), 0)
        for t in ticks:
            lo = t - (N - 1) if t >= N else 0                    # the oldest sample leaves before tick t is predicted
            if t > 0:
                f = mo.fit(kid, theta[w], xs[w, lo:t], ys[w, lo:t])
                mu, var = mo.predict(f, xs[w, t:t + 1])
                assert abs(pm[w, t] - mu[0]) <= TOL * max(abs(mu[0]), np.max(np.abs(ys[w]))) and abs(pv[w, t] - var[0]) <= TOL * var[0]
            lo2 = max(0, t + 1 - N)
            f = mo.fit(kid, theta[w], xs[w, lo2:t + 1], ys[w, lo2:t + 1])
            assert abs(lm[w, t] - f.logml) <= TOL * max(abs(f.logml), 1.0)
    return ctx, xs_all, ys_all, theta


@pytest.mark.parametrize("kid", KIDS)
def test_window_stream_small_against_full_refit_stream(engine, kid):
    """8 windows x N = 96, 2 000 ticks in uneven blocks (filling, full, across ring compactions): two windows against the refit
    stream at every tick, the rest at checkpoints."""
    nwin, N, d, T = 8, 96, 2, 2000
    cuts = [0, 50, 51, 96, 97, 400, 1203, T]
    ctx, xs, ys, theta = check_stream(engine, kid, nwin, N, d, T, cuts, range(nwin), (0, 1, 95, 96, 97, 500, 1203, T - 1))
    xs2, ys2 = stream(T, d, 5 * N + kid, nwin)
    w = 3
    xs_b, ys_b = xs2[w, :400], ys2[w, :400]
    ctx2 = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx2.window_init(1, N, d, kid, theta[w])
    pm, pv, lm = (o[0] for o in ctx2.window_push(xs_b[None], ys_b[None]))
    opm, opv, olm = mo.sliding_window_stream(kid, theta[w], N, xs_b, ys_b)
    assert rel(pm, opm) < TOL and relv(pv, opv) < TOL and np.max(np.abs(lm - olm) / np.maximum(np.abs(olm), 1.0)) < TOL


@pytest.mark.parametrize("kid,nwin,N,T", [(3, 64, 512, 600), (4, 64, 512, 600), (4, 512, 64, 203)])
def test_window_stream_many_windows(engine, kid, nwin, N, T):
    """64 x N = 512 (paired passes) and 512 x N = 64 (four-tick passes), blocks cut so that single-tick passes occur too."""
    check_stream(engine, kid, nwin, N, 3, T, [0, 1, 130, T - 1, T], (0, nwin // 2, nwin - 1), (0, 1, 63, 64, 129, T - 2, T - 1))


@pytest.mark.parametrize("kid", KIDS)
def test_window_forecast_joint_sample_set_theta_grad_optimize(engine, kid):
    nwin, N, d, T, M = 6, 80, 2, 190, 37
    ctx, xs3, ys3, theta = check_stream(engine, kid, nwin, N, d, T, [0, T], (0, 5), (T - 1,), extra=40)
    xs, ys = xs3[:, :T], ys3[:, :T]
    rng = np.random.default_rng(3)
    Xq = rng.normal(size=(nwin, M, d)) * 0.5 + xs[:, -1:, :]
    mean, var = ctx.window_predict(Xq)
    ctx.window_joint_reserve(M)
    mj, cov = ctx.window_predict_cov(Xq)
    fits = [mo.fit(kid, theta[w], xs[w, T - N:], ys[w, T - N:]) for w in range(nwin)]
    for w in range(nwin):
        omu, ocov = mo.predict_cov(fits[w], Xq[w])
        assert rel(mean[w], omu) < TOL and relv(var[w], np.diag(ocov)) < TOL
        assert rel(mj[w], omu) < TOL and rel(cov[w], ocov) < TOL and np.array_equal(cov[w], cov[w].T)
    # sample paths with unit-vector draws: column m of the factor of (latent covariance + jitter)
    xi = np.tile(np.eye(M)[None, :5], (nwin, 1, 1))
    paths, sinfo = ctx.window_sample(Xq, xi, include_noise=False, jitter_rel=1e-6)
    assert not sinfo.any()
    for w in (0, 5):
        _, oc = mo.predict_cov(fits[w], Xq[w], include_noise=False)
        C = np.linalg.cholesky(oc + 1e-6 * np.mean(np.diag(oc)) * np.eye(M))
        assert rel(paths[w] - mj[w][None], C[:, :5].T) < 1e-5
    # the gradient of the resident windows = cgp_nll_grad on a host copy
    nll, g = ctx.window_nll_grad()
    host = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=nwin)
    for w in range(nwin):
        n1, g1 = host.nll_grad(xs[w, T - N:], ys[w, T - N:], kid, theta[w])
        assert abs(nll[w] - n1) <= TOL * max(abs(n1), 1.0) and rel(g[w], g1) < TOL
    # a new length-scale mid-stream, then more ticks
    th2 = theta.copy()
    th2[:, 1] *= 1.7
    logml, info = ctx.window_set_theta(th2)
    assert not info.any()
    for w in range(nwin):
        assert abs(logml[w] - mo.fit(kid, th2[w], xs[w, T - N:], ys[w, T - N:]).logml) <= TOL * max(abs(logml[w]), 1.0)
    pm, pv, lm = ctx.window_push(xs3[:, T:], ys3[:, T:])
    w = 2
    f = mo.fit(kid, th2[w], xs3[w, T + 40 - N:], ys3[w, T + 40 - N:])
    assert abs(lm[w, -1] - f.logml) <= TOL * max(abs(f.logml), 1.0)
    # optimiser of the resident windows = cgp_optimize_batch on the host copy, from the same start
    tho, lo, nev = ctx.window_optimize()
    thb, lb, nb = host.optimize_batch(xs3[:, T + 40 - N:], ys3[:, T + 40 - N:], kid, th2)
    assert np.max(np.abs(lo - lb) / np.maximum(np.abs(lb), 1.0)) < TOL


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_fp32_contexts_refuse_matern_and_stay_usable(engine):
    X, y, Xs, th = window(1, 64, 2, 9)
    ctx = engine.Context(max_n=64, max_m=64, max_d=2, max_batch=2, dtype=engine.F32)
    lib, h, p = ctx.lib, ctx.h, engine._p
    for kid in KIDS:
        import ctypes
        dbl, out = ctypes.c_double(0.0), np.zeros(64)
        info, nev, mo_ = np.zeros(2, dtype=np.int32), ctypes.c_int(0), ctypes.c_int(0)
        th2 = np.ascontiguousarray(np.tile(th, (2, 1)))
        t, s = np.arange(1.0, 41.0), np.linspace(0.0, 0.3, 40)
        rcs = [lib.cgp_fit(h, p(X), p(y), 64, 2, kid, p(th), ctypes.byref(dbl)),
               lib.cgp_fit_predict_batch(h, 1, 64, 2, 9, kid, p(X), p(y), p(Xs), p(th), 4, 1, p(out), p(out), p(out), info.ctypes.data_as(engine._ip)),
               lib.cgp_nll_grad(h, p(X), p(y), 64, 2, kid, p(th), ctypes.byref(dbl), p(out)),
               lib.cgp_optimize(h, p(X), p(y), 64, 2, kid, p(th.copy()), 10, ctypes.byref(dbl), ctypes.byref(nev)),
               lib.cgp_optimize_batch(h, 1, 64, 2, kid, p(X), p(y), p(th2), 4, 10, p(out), info.ctypes.data_as(engine._ip)),
               lib.cgp_slip_node_callback(h, p(t), p(s), 40, kid, p(np.ones(3)), p(np.zeros(700)), p(np.zeros(700)), 700, ctypes.byref(mo_)),
               lib.cgp_slip_node_callback_opt(h, p(t), p(s), 40, kid, p(np.ones(3)), 10, p(np.zeros(700)), p(np.zeros(700)), 700, ctypes.byref(mo_)),
               lib.cgp_window_init(h, 2, 32, 2, kid, p(th2), 4)]
        assert rcs == [-1] * len(rcs), rcs
    rc, logml = ctx.fit(X, y, 1, th)                     # the context is still usable
    assert rc == 0 and abs(logml - go.fit(1, th, X, y).logml) < 1e-3 * abs(logml)


def test_unknown_kernel_and_short_theta_stride_are_einval(engine):
    import ctypes
    X, y, Xs, th = window(2, 32, 3, 5)
    ctx = engine.Context(max_n=32, max_m=32, max_d=3, max_batch=2)
    lib, h, p = ctx.lib, ctx.h, engine._p
    dbl, out, info = ctypes.c_double(0.0), np.zeros(32), np.zeros(2, dtype=np.int32)
    assert lib.cgp_fit(h, p(X), p(y), 32, 3, 5, p(th), ctypes.byref(dbl)) == -1
    assert lib.cgp_window_init(h, 1, 16, 3, 5, p(th), 5) == -1
    for kid in KIDS:
        assert lib.cgp_fit_predict_batch(h, 1, 32, 3, 5, kid, p(X), p(y), p(Xs), p(th), 4, 1, p(out), p(out), p(out),
                                         info.ctypes.data_as(engine._ip)) == -1
        assert lib.cgp_window_init(h, 1, 16, 3, kid, p(th), 4) == -1
        assert lib.cgp_fit(h, p(X), p(y), 32, 3, kid, p(th), ctypes.byref(dbl)) == 0


# ---- the kernels that were there before compute what they computed -----------------------------------------------------------
def legacy_outputs(engine, which):
    """One SE_ARD batch (tiled schedules) and the reference's RBF x Brownian window (short-window kernels, node callback,
    sliding windows): every array a caller receives."""
    if which == "se_ard":
        z = np.load(os.path.join(GOLDEN, "sk_se_ard_n256_d6.npz"))
        X, y, Xs, th = z["X"], z["y"], z["Xs"], z["theta"]
        ctx = engine.Context(max_n=256, max_m=256, max_d=6, max_batch=70)
        B = 70
        sc = np.linspace(0.7, 1.3, B)
        rc, mean, var, logml, info = ctx.fit_predict_batch(np.tile(X, (B, 1, 1)), y[None] * sc[:, None], np.tile(Xs, (B, 1, 1)),
                                                           np.tile(th, (B, 1)), 1)
        rc1, l1 = ctx.fit(X, y, 1, th)
        m1, v1 = ctx.predict(Xs)
        nll, g = ctx.nll_grad(X, y, 1, th)
        ctx.window_init(3, 48, 6, 1, th)
        pm, pv, lm = ctx.window_push(np.stack([X[:150], X[50:200], X[100:250]]), np.stack([y[:150], y[50:200], y[100:250]]))
        fm, fv = ctx.window_predict(np.tile(Xs[:20], (3, 1, 1)))
        return np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in (mean, var, logml, [l1], m1, v1, ctx.alpha(), [nll], g, pm, pv, lm, fm, fv)])
    z = np.load(os.path.join(GOLDEN, "slipval_window_rbfbrownian.npz"))
    t, s, th = z["time_array"], z["slip_array"], z["theta"]
    ctx = engine.Context(max_n=256, max_m=1024, max_d=1, max_batch=4)
    m, sg = ctx.slip_node_callback(t, s, th)
    nll, g = ctx.nll_grad(t[:134], s[:134], 2, th)
    tho, lo, nev = ctx.optimize(t[:134], s[:134], 2, np.ones(4))
    big = engine.Context(max_n=200, max_m=700, max_d=1, max_batch=2)      # more than 160 samples: the tiled route
    ta, sa = z["all_ticks"].astype(np.float64), z["all_slip"].astype(np.float64)
    rc, logml = big.fit(ta[:, None], sa, 2, th)
    bm, bv = big.predict((ta[-1] + 1.0 + np.arange(599.0))[:, None])
    ctx.window_init(1, 40, 1, 2, th)
    pm, pv, lm = ctx.window_push(t[None, :, None], s[None])
    return np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in (m, sg, [nll], g, tho, [lo, nev], [logml], bm, bv, pm, pv, lm)])


@pytest.mark.parametrize("which", ["se_ard", "rbf_brownian"])
def test_existing_kernels_reproduce_recorded_outputs_bitwise(engine, which):
    want = np.load(os.path.join(GOLDEN, f"pre_matern_{which}.npy"))
    got = legacy_outputs(engine, which)
    assert got.shape == want.shape and np.array_equal(got, want)


if __name__ == "__main__" and "--record" in sys.argv:
    import corenav_gp_amd.engine as eng
    eng.load()
    out = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    os.makedirs(out, exist_ok=True)
    for name in ("se_ard", "rbf_brownian"):
        np.save(os.path.join(out, f"pre_matern_{name}.npy"), legacy_outputs(eng, name))
        print("recorded", name)
