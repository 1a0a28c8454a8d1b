"""GPU parity of the sliding windows' predictive gradients (cgp_window_predict_gradients[_device]: d mean / d x* and d var / d x*
at M test points from the factor, z, alpha and inputs the pushes maintain) against tests/window_pgrad_oracle.py, which refits the
window's samples from scratch.  Bar: the project's fp64 bar, 1e-6, measured as in tests/test_gpu_pgrad.py: per window
max|dmean - oracle| / max|oracle dmean|, and the same for dvar.  Largest errors measured on the parity cases below, per kernel
id (dmean / dvar): DESIGN.md section 9g."""
import numpy as np
import pytest

import pgrad_oracle as po
import window_pgrad_oracle as wo
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h
WORST = {}                # kernel id -> [dmean, dvar] largest error seen, printed by the parity tests


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
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def points_for(kid, X, t, N, M, rng):
    """RBF x Brownian: a third of the points on the ticks after the last sample (the reference's grid), a third on the ticks
    inside the window (ties), a third inside it off the ticks; else points around the window's inputs."""
    if kid == 2:
        last, lo = X[max(t, 1) - 1, 0], X[max(t - N, 0), 0]
        after = last + 1.0 + np.arange(M, dtype=np.float64)
        on = np.floor(rng.uniform(lo, last + 1.0, size=M))
        off = on + rng.uniform(0.1, 0.9, size=M)
        pick = rng.integers(0, 3, size=M) if M > 1 else np.array([0])
        return np.where(pick == 0, after, np.where(pick == 1, on, off))[:, None]
    lo = max(0, t - 50)
    return X[rng.integers(lo, max(t, 1), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def errors(dmean, dvar, odm, odv):
    return (np.max(np.abs(dmean - odm)) / max(np.max(np.abs(odm)), 1e-300), np.max(np.abs(dvar - odv)) / max(np.max(np.abs(odv)), 1e-300))


def close(dmean, dvar, kid, theta, N, X, y, Xs, what=""):
    odm, odv = wo.sliding_window_gradients(kid, theta, N, X, y, Xs)
    em, ev = errors(dmean, dvar, odm, odv)
    w = WORST.setdefault(kid, [0.0, 0.0])
    w[0], w[1] = max(w[0], em), max(w[1], ev)
    print(f"{what} kid {kid} errors / bar: dmean {em / TOL:.3g} dvar {ev / TOL:.3g}")
    assert em <= TOL and ev <= TOL, (what, em, ev)


def new_ctx(engine, d):
    return engine.Context(max_n=8, max_m=8, max_d=d)


PARITY = [(2, 16, 1), (2, 17, 1), (2, 40, 1), (0, 33, 2), (1, 64, 3), (1, 100, 6), (1, 48, 8), (3, 40, 2), (4, 64, 3)]


@pytest.mark.parametrize("kid,N,d", PARITY)
def test_gradients_match_refit_oracle(engine, kid, N, d):
    """M = 1, 33 and 599 at the moments t = 0 (empty: the prior rule, exactly), 1, N // 2 (filling), N - 3 (n no multiple of 16),
    N, 2N - 1, 2N, 2N + 1 (either side of the ring's compaction; an origin that is no multiple of 16) and 3N + 6 (two turnovers)
    of one stream; mean / var are bitwise cgp_window_predict's, with include_noise both ways."""
    T = 3 * N + 6
    X, y = stream(T, d, 100 + N)
    theta = theta_of(kid, d)
    rng = np.random.default_rng(N)
    ctx = new_ctx(engine, d)
    ctx.window_init(1, N, d, kid, theta)
    fed = 0
    for t in (0, 1, N // 2, N - 3, N, 2 * N - 1, 2 * N, 2 * N + 1, T):
        if t > fed:
            ctx.window_push(X[fed:t][None], y[fed:t][None])
            fed = t
        assert ctx.window_state(0) == (min(N, t), 0)
        for M in (1, 33, 599):
            Xs = points_for(kid, X, t, N, M, rng)
            if t == 0 and kid == 2 and M >= 3:
                Xs[:3, 0] = (-4.0, 0.0, 7.0)
            for noise in (True, False):
                mean, var, dmean, dvar = ctx.window_predict_gradients(Xs, include_noise=noise)
                assert mean.shape == var.shape == (1, M) and dmean.shape == dvar.shape == (1, M, d)
                pm, pv = ctx.window_predict(Xs, include_noise=noise)
                assert np.array_equal(mean, pm) and np.array_equal(var, pv)
                if noise:
                    first = (dmean, dvar)
                else:   # include_noise only affects var
                    assert np.array_equal(first[0], dmean) and np.array_equal(first[1], dvar)
            if t == 0:
                odm, odv = wo.sliding_window_gradients(kid, theta, N, X[:0], y[:0], Xs)
                assert np.all(dmean == 0.0) and np.array_equal(dvar[0], odv)
                kdiag = po.mo.kernel_Kdiag if kid in po.mo.KERNELS else po.go.kernel_Kdiag
                assert np.all(mean == 0.0)
                np.testing.assert_allclose(var[0], kdiag(kid, theta, Xs), rtol=1e-14)   # (the last call had include_noise = False)
            else:
                close(dmean[0], dvar[0], kid, theta, N, X[:t], y[:t], Xs, what=f"t {t} M {M}")
    print("largest errors so far, kernel id -> (dmean, dvar):", {k: tuple(v) for k, v in WORST.items()})


@pytest.mark.parametrize("N,d,M,T", [(700, 3, 17, 1500), (1536, 2, 9, 1700)])
def test_the_two_longer_forms(engine, N, d, M, T):
    """512 < N <= 1024 (sixteen test points per workgroup) and N > 1024 (eight): M one past each chunk width."""
    X, y = stream(T, d, N)
    theta = theta_of(1, d)
    rng = np.random.default_rng(4)
    ctx = new_ctx(engine, d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, N, M, rng)
    mean, var, dmean, dvar = ctx.window_predict_gradients(Xs)
    pm, pv = ctx.window_predict(Xs)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    close(dmean[0], dvar[0], 1, theta, N, X, y, Xs, what=f"N {N}")


def three_windows(kid=1, W=3, N=40, d=3, T=100, M=53, seed=500):
    rng = np.random.default_rng(seed)
    Xw, yw = zip(*[stream(T, d, seed + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    Xs = X[:, rng.integers(T - N, T, size=M)] + 0.2 * rng.normal(size=(W, M, d))
    return X, y, theta_of(kid, d), Xs


def test_host_device_and_graph_replay_agree_bitwise(engine):
    import torch
    W, N, d, M = 3, 40, 3, 53
    X, y, theta, Xs = three_windows()
    ctx = new_ctx(engine, d)
    ctx.window_init(W, N, d, 1, theta)
    ctx.window_push(X, y)
    ref = ctx.window_predict_gradients(Xs)
    dxs = torch.from_numpy(Xs).cuda()
    out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((W, M), (W, M), (W, M, d), (W, M, d))]

    def clear():
        for t in out:
            t.fill_(-1.0)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        for t, r in zip(out, ref):
            assert np.array_equal(t.cpu().numpy(), r)

    def enqueue(s):
        assert ctx.window_predict_gradients_device(M, dxs.data_ptr(), True, *[t.data_ptr() for t in out], stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()


def test_null_outputs_leave_the_others_bit_identical(engine):
    W, N, d, M = 3, 40, 3, 53
    X, y, theta, Xs = three_windows()
    ctx = new_ctx(engine, d)
    ctx.window_init(W, N, d, 1, theta)
    ctx.window_push(X, y)
    mean, var, dmean, dvar = ctx.window_predict_gradients(Xs)
    full = dict(mean=mean, var=var, dmean=dmean, dvar=dvar)
    for moments in (("mean",), ("var",), ()):
        for want in (("dmean", "dvar"), ("dmean",), ("dvar",)):
            got = dict(zip(("mean", "var", "dmean", "dvar"), ctx.window_predict_gradients(Xs, want=want, moments=moments)))
            for k, v in got.items():
                if k in moments or k in want:
                    assert np.array_equal(v, full[k]), (moments, want, k)
                else:
                    assert v is None


def test_slot_and_neighbour_independence(engine):
    """Five windows fed permuted copies of three streams: each equals the same stream alone in a one-window context.  (The
    windows are brought to their state tick by tick: a one-tick push is the single-tick kernel whatever the context.)"""
    N, d, M, T = 40, 2, 45, 70
    rng = np.random.default_rng(31)
    Xw, yw = zip(*[stream(T, d, 800 + w) for w in range(3)])
    Xq = [Xw[k][rng.integers(T - N, T, size=M)] + 0.2 * rng.normal(size=(M, d)) for k in range(3)]
    th3 = np.stack([theta_of(1, d) * (1.0 + 0.1 * k) for k in range(3)])
    slots = [2, 0, 1, 0, 2]
    X, y, Xs, theta = (np.stack([a[k] for k in slots]) for a in (Xw, yw, Xq, th3))
    big = new_ctx(engine, d)
    big.window_init(5, N, d, 1, theta)
    alone = []
    for k in range(3):
        c = new_ctx(engine, d)
        c.window_init(1, N, d, 1, th3[k])
        alone.append(c)
    for i in range(T):
        big.window_push(X[:, i:i + 1], y[:, i:i + 1])
        for k in range(3):
            alone[k].window_push(Xw[k][None, i:i + 1], yw[k][None, i:i + 1])
    got = big.window_predict_gradients(Xs)
    for k in range(3):
        one = alone[k].window_predict_gradients(Xq[k])
        for w in [s for s in range(5) if slots[s] == k]:
            for a, b in zip(got, one):
                assert np.array_equal(a[w], b[0]), (k, w)


def test_gradients_do_not_touch_the_windows(engine):
    """push A, gradients, push B = push A, push B on a second context, bitwise (outputs of B and a forecast after it)."""
    N, d, T = 48, 2, 170
    X, y = stream(T, d, 77)
    theta = theta_of(1, d)
    rng = np.random.default_rng(1)
    Xs = points_for(1, X, T, N, 70, rng)
    outs = []
    for between in (True, False):
        ctx = new_ctx(engine, d)
        ctx.window_init(1, N, d, 1, theta)
        ctx.window_push(X[:90][None], y[:90][None])
        if between:
            ctx.window_predict_gradients(Xs)
            ctx.window_predict_gradients(Xs[:3], include_noise=False, want=("dvar",))
        outs.append(ctx.window_push(X[90:][None], y[90:][None]) + ctx.window_predict(Xs))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_shared_scratch_carries_no_state(engine):
    """After a gradient call, window_nll_grad, window_loo, window_predict and window_predict_cov return bitwise what they
    return without it, and the gradient call after each of them returns bitwise what it returned first."""
    W, N, d, M = 3, 40, 3, 53
    X, y, theta, Xs = three_windows()
    others = {"nll_grad": lambda c: c.window_nll_grad(), "loo": lambda c: c.window_loo(),
              "predict": lambda c: c.window_predict(Xs), "predict_cov": lambda c: c.window_predict_cov(Xs)}

    def fresh():
        c = new_ctx(engine, d)
        c.window_init(W, N, d, 1, theta)
        c.window_push(X, y)
        c.window_joint_reserve(M)
        return c

    plain = fresh()
    before = {k: f(plain) for k, f in others.items()}
    ctx = fresh()
    first = ctx.window_predict_gradients(Xs)
    for k, f in others.items():
        got = f(ctx)
        for a, b in zip(got, before[k]):
            assert np.array_equal(a, b, equal_nan=True), k
        again = ctx.window_predict_gradients(Xs)
        for a, b in zip(again, first):
            assert np.array_equal(a, b), k


def test_failed_window_answers_nan_and_the_others_are_unaffected(engine):
    """Window 1 of three has sigma_n^2 < -sigma_f^2 (the set-up of the forecast's test of the same name): NaN in all four of
    its outputs, the host form returns its tick code, the neighbours are at parity; after window_set_theta revives it its
    gradients meet the oracle."""
    W, N, d, T, M = 3, 24, 1, 30, 40
    Xw, yw = zip(*[stream(T, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    theta[1, -1] = -2.0 * theta[1, 0]
    rng = np.random.default_rng(2)
    Xs = X[:, -1:, :] + rng.random((W, M, 1)) * 5.0
    ctx = new_ctx(engine, d)
    ctx.window_init(W, N, d, 0, theta)
    with pytest.raises(engine.CgpError):
        ctx.window_push(X, y)
    code = ctx.window_state(1)[1]
    assert code > 0 and ctx.window_state(0)[1] == 0 and ctx.window_state(2)[1] == 0
    mean, var, dmean, dvar, rc = ctx.window_predict_gradients(Xs, check=False)
    assert rc == code
    with pytest.raises(engine.CgpError):
        ctx.window_predict_gradients(Xs)
    for a in (mean, var, dmean, dvar):
        assert np.all(np.isnan(a[1])) and not np.any(np.isnan(a[[0, 2]]))
    for w in (0, 2):
        close(dmean[w], dvar[w], 0, theta[w], N, X[w], y[w], Xs[w], what=f"neighbour {w}")
    good = np.tile(theta_of(0, d), (W, 1))
    ctx.window_set_theta(good, select=np.array([0, 1, 0], dtype=np.uint8))
    mean, var, dmean, dvar = ctx.window_predict_gradients(Xs)
    for w in range(W):
        close(dmean[w], dvar[w], 0, good[w], N, X[w], y[w], Xs[w], what=f"revived, window {w}")


def test_two_device_paths_agree_on_a_full_window(engine):
    """A full N = 192 window (d = 3, SE-ARD) against cgp_fit_predict_grad_batch on the same 192 samples: the windows' kernels
    and the fit schedule's, fp64 both, within the 1e-6 bar."""
    N, d, T, M = 192, 3, 450, 70
    X, y = stream(T, d, 192)
    theta = theta_of(1, d)
    rng = np.random.default_rng(8)
    Xs = points_for(1, X, T, N, M, rng)
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=1)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    _, _, dmean, dvar = ctx.window_predict_gradients(Xs)
    assert ctx.pgrad_reserve(1, M) == 0
    rc, _, _, _, info, bdm, bdv = ctx.fit_predict_grad_batch(X[None, T - N:], y[None, T - N:], Xs[None], theta[None], 1)
    assert rc == 0 and info[0] == 0
    em, ev = errors(dmean[0], dvar[0], bdm[0], bdv[0])
    print(f"windows against the fit schedule: dmean {em:.3g} dvar {ev:.3g}")
    assert em <= TOL and ev <= TOL, (em, ev)


def test_dmean_is_the_central_difference_of_the_windows_own_mean(engine):
    """Step 1e-5; the tolerance is 10 x the error the same differences show on the oracle at the same points (computed here)."""
    N, d, T, M, h = 64, 3, 150, 20, 1e-5
    X, y = stream(T, d, 64)
    theta = theta_of(1, d)
    rng = np.random.default_rng(6)
    Xs = points_for(1, X, T, N, M, rng)
    ctx = new_ctx(engine, d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    _, _, dmean, _ = ctx.window_predict_gradients(Xs, want=("dmean",))
    f = wo.window_fit(1, theta, N, X, y)
    odm, _ = po.predictive_gradients(f, Xs)
    fd, ofd = np.empty((M, d)), np.empty((M, d))
    for q in range(d):
        e = np.zeros(d)
        e[q] = h
        fd[:, q] = (ctx.window_predict(Xs + e)[0][0] - ctx.window_predict(Xs - e)[0][0]) / (2 * h)
        ofd[:, q] = (po.unclipped_mean_var(f, Xs + e)[0] - po.unclipped_mean_var(f, Xs - e)[0]) / (2 * h)
    scale = np.max(np.abs(odm))
    oerr = np.max(np.abs(ofd - odm)) / scale
    err = np.max(np.abs(fd - dmean[0])) / scale
    print(f"central differences: the windows {err:.3g}, the oracle {oerr:.3g}")
    assert err <= 10 * oerr, (err, oerr)


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    buf = np.zeros(8)
    p, a = engine._p(buf), buf.ctypes.data
    lib = ctx.lib
    assert lib.cgp_window_predict_gradients(ctx.h, 1, p, 1, p, p, p, p) == ESTATE
    assert lib.cgp_window_predict_gradients_device(ctx.h, 1, a, 1, a, a, a, a, None) == ESTATE
    ctx.window_init(1, 8, 1, 2, theta_of(2, 1))
    assert lib.cgp_window_predict_gradients(ctx.h, 0, p, 1, p, p, p, p) == EINVAL
    assert lib.cgp_window_predict_gradients_device(ctx.h, 0, a, 1, a, a, a, a, None) == EINVAL
    assert lib.cgp_window_predict_gradients(ctx.h, 1, None, 1, p, p, p, p) == EINVAL
    assert lib.cgp_window_predict_gradients_device(ctx.h, 1, None, 1, a, a, a, a, None) == EINVAL
    assert lib.cgp_window_predict_gradients(ctx.h, 1, p, 1, p, p, None, None) == EINVAL
    assert lib.cgp_window_predict_gradients_device(ctx.h, 1, a, 1, a, a, None, None, None) == EINVAL
    # the context stays usable
    X, y = stream(12, 1, 3)
    ctx.window_push(X[None], y[None])
    Xs = X[-1:] + 1.0 + np.arange(5.0)[:, None]
    _, _, dmean, dvar = ctx.window_predict_gradients(Xs)
    close(dmean[0], dvar[0], 2, theta_of(2, 1), 8, X, y, Xs)
