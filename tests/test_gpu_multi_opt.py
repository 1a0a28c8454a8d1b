"""GPU tests of the multi-target objective (cgp_multi_nll_grad_batch[_device], cgp_optimize_multi_batch: value, gradient and
optimiser of -sum_p logml[p] over one shared theta, from one factorisation per fit) against the per-column oracle
(tests/multi_opt_oracle.py), through engine.py.  Bars are the project's: 1e-6 for nll (relative) and for the gradient against
max|grad| (test_gpu_optimize.py::test_nll_grad_matches_oracle), logml against max(1, |logml|) (multi_oracle.errors); 1e-9 between
two device routes; SURVEY 8c for optima; bitwise wherever the header promises it.  Windows are test_gpu_multi.py's recipe.  Shapes
sit on the tile edges: 128-sample block columns, the 16-column chunks of the rank-P loop, the 64 / 128 row tiles of the solve, the
128-target tiles of k_multi_alpha."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import multi_opt_oracle as moo
from multi_oracle import fit_predict_multi, errors
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def window(N, d, P, seed, tick0=11):
    """test_gpu_multi.py::window: P slip series on the one time base, a seed per column."""
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1)), t) for p in range(P)])
    if d == 1:
        return t[:, None], Y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)]), Y


def problem(B, N, d, P, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, Yw = zip(*[window(N, d, P, seed + 17 * b, tick0=11 + b) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return np.stack(Xw), np.stack(Yw), theta


def ctx_for(engine, B, N, d, P, max_m=None):
    ctx = engine.Context(max_n=N, max_m=max_m or N, max_d=d, max_batch=B)
    assert ctx.multi_reserve(B, P) == 0 and ctx.multi_grad_reserve(B, P) == 0
    return ctx


def close(kid, theta, X, Y, nll, grad, logml, tol=TOL, what=""):
    onll, og, ol = moo.nll_and_grad_multi(kid, theta, X, Y)
    en = abs(nll - onll) / abs(onll)
    eg = np.max(np.abs(grad - og)) / np.max(np.abs(og))
    el = np.max(np.abs(logml - ol) / np.maximum(1.0, np.abs(ol)))
    print(f"{what}errors / bar: nll {en / tol:.3g} grad {eg / tol:.3g} logml {el / tol:.3g}")
    assert en <= tol and eg <= tol and el <= tol, (en, eg, el)


@pytest.mark.parametrize("kid,d", [(0, 3), (1, 3), (1, 8), (2, 1), (3, 3), (4, 3)])
def test_every_kernel(engine, kid, d):
    B, N, P = 2, 130, 3
    X, Y, theta = problem(B, N, d, P, kid, 10 * kid + d)
    ctx = ctx_for(engine, B, N, d, P)
    rc, nll, grad, logml, info = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc == 0 and not info.any() and nll.shape == (B,) and grad.shape == theta.shape and logml.shape == (B, P)
    for b in range(B):
        close(kid, theta[b], X[b], Y[b], nll[b], grad[b], logml[b])
        assert nll[b] == pytest.approx(-np.sum(logml[b]), rel=1e-13)


@pytest.mark.parametrize("N,P", [(128, 1), (129, 15), (129, 16), (257, 17), (257, 64), (129, 65), (257, 129)])
def test_tile_edges(engine, N, P):
    B, d, kid = 2, 2, 1
    X, Y, theta = problem(B, N, d, P, kid, N * P)
    ctx = ctx_for(engine, B, N, d, P)
    outs = {}
    for rows in (64, 128):
        assert ctx.multi_set_form(rows) == 0
        rc, nll, grad, logml, info = ctx.multi_nll_grad_batch(X, Y, theta, kid)
        assert rc == 0 and not info.any()
        outs[rows] = (nll, grad, logml)
    for a, b in zip(outs[64], outs[128]):   # both forms of the solve: the same Z, so the same bits after it
        assert np.array_equal(a, b)
    b = 1   # one fit against P oracle evaluations
    close(kid, theta[b], X[b], Y[b], nll[b], grad[b], logml[b])


def test_one_target_is_cgp_nll_grad(engine):
    """P = 1 against cgp_nll_grad of that column (N = 257: the tiled machinery on both sides): other sums, 1e-9."""
    B, N, d, kid = 2, 257, 3, 1
    X, Y, theta = problem(B, N, d, 1, kid, 5)
    ctx = ctx_for(engine, B, N, d, 1)
    rc, nll, grad, _, _ = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc == 0
    one = engine.Context(max_n=N, max_m=N, max_d=d)
    for b in range(B):
        n1, g1 = one.nll_grad(X[b], Y[b, 0], kid, theta[b])
        assert abs(nll[b] - n1) <= 1e-9 * abs(n1) and np.max(np.abs(grad[b] - g1)) <= 1e-9 * np.max(np.abs(g1))


def test_two_targets_are_the_sum_of_two_calls(engine):
    B, N, d, kid = 2, 257, 3, 4
    X, Y, theta = problem(B, N, d, 2, kid, 6)
    ctx = ctx_for(engine, B, N, d, 2)
    rc, nll, grad, logml, _ = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc == 0
    parts = [ctx.multi_nll_grad_batch(X, Y[:, [p]], theta, kid) for p in range(2)]
    assert parts[0][0] == 0 and parts[1][0] == 0
    sn, sg = parts[0][1] + parts[1][1], parts[0][2] + parts[1][2]
    assert np.max(np.abs(nll - sn) / np.abs(sn)) <= 1e-9
    assert np.max(np.max(np.abs(grad - sg), axis=1) / np.max(np.abs(sg), axis=1)) <= 1e-9
    for p in range(2):   # a column's logml does not see the other column
        assert np.array_equal(logml[:, p], parts[p][3][:, 0])


@pytest.mark.parametrize("B", [3, 30])   # the latency and the mid-size schedule
def test_slot_and_neighbour_independence(engine, B):
    """Fit 1's window also sits in the last slot; a second call of the same size has other neighbours and the window in slot 0."""
    N, d, P, kid = 257, 2, 5, 1
    X, Y, theta = problem(B, N, d, P, kid, 7 + B)
    X[-1], Y[-1], theta[-1] = X[1], Y[1], theta[1]
    ctx = ctx_for(engine, B, N, d, P)
    out = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    X2, Y2, theta2 = problem(B, N, d, P, kid, 1007 + B)
    X2[0], Y2[0], theta2[0] = X[1], Y[1], theta[1]
    out2 = ctx.multi_nll_grad_batch(X2, Y2, theta2, kid)
    assert out[0] == 0 and out2[0] == 0
    for u, w in zip(out[1:4], out2[1:4]):
        assert np.array_equal(u[1], u[B - 1]) and np.array_equal(u[1], w[0])
    close(kid, theta[1], X[1], Y[1], out[1][1], out[2][1], out[3][1])


def device_arrays(torch, X, Y, theta):
    th = np.zeros((X.shape[0], 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), Y, th)]


def device_outputs(torch, B, P, stride):
    f = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    return f(B), f(B, stride), f(B, P), torch.empty(B, dtype=torch.int32, device="cuda")


def test_host_device_and_graph_replay_agree_bitwise(engine):
    """The host call, the device call on the legacy stream and on the context's, and two replays of a captured side stream; the
    device gradient in rows of another stride, and without a logml buffer."""
    import torch
    B, N, d, P, kid, stride = 2, 257, 3, 9, 1, 7
    X, Y, theta = problem(B, N, d, P, kid, 10)
    nth = theta.shape[1]
    ctx = ctx_for(engine, B, N, d, P)
    rc, nll, grad, logml, _ = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc == 0
    dX, dY, dth = device_arrays(torch, X, Y, theta)
    outs = device_outputs(torch, B, P, stride)
    ptrs = [t.data_ptr() for t in outs]

    def clear():
        for t in outs[:3]:
            t.fill_(-1.0)
        outs[3].fill_(-1)
        torch.cuda.synchronize()

    def check(with_logml=True):
        ctx.synchronize()
        torch.cuda.synchronize()
        g = outs[1].cpu().numpy()
        assert np.array_equal(outs[0].cpu().numpy(), nll) and np.array_equal(g[:, :nth], grad) and np.all(g[:, nth:] == -1.0)
        assert np.array_equal(outs[2].cpu().numpy(), logml if with_logml else np.full((B, P), -1.0))
        assert not outs[3].cpu().numpy().any()

    def enqueue(s, with_logml=True):
        assert ctx.multi_nll_grad_batch_device(B, N, d, P, kid, dX.data_ptr(), dY.data_ptr(), dth.data_ptr(), 0, ptrs[0], ptrs[1],
                                               stride, ptrs[2] if with_logml else 0, ptrs[3], stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    clear()
    enqueue(0, with_logml=False)
    check(with_logml=False)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()


def ladder_problem():
    """Fit 1: duplicated inputs and sigma_n^2 = 1e-10 under a large amplitude -- Ky does not factor without jitter."""
    rng = np.random.default_rng(21)
    N, d, B, P = 200, 1, 3, 3
    X = np.stack([np.sort(rng.normal(size=(N, d)), 0) for _ in range(B)])
    Xgood = X.copy()
    X[1, :, 0] = np.repeat(np.arange(N // 2, dtype=float), 2)
    cols = lambda x: np.stack([np.sin(x), np.cos(x), np.sin(2.0 * x) + 0.5], axis=1)   # (B, P, N)
    th = np.array([[1.0, 1.0, 0.05], [1e9, 3.0, 1e-10], [1.0, 1.0, 0.05]])
    thgood = np.array([[1.0, 1.0, 0.05]] * 3)
    return X, cols(X[:, :, 0]), th, Xgood, cols(Xgood[:, :, 0]), thgood


def test_jitter_ladder_is_per_fit(engine):
    X, Y, th, Xgood, Ygood, thgood = ladder_problem()
    B, N, d = X.shape
    P = Y.shape[1]
    assert go.fit(0, th[1], X[1], Y[1, 0]).jitter > 0
    ctx = ctx_for(engine, B, N, d, P)
    rc, nll, grad, logml, info = ctx.multi_nll_grad_batch(X, Y, th, 0)
    assert rc == 0 and not info.any()
    close(0, th[1], X[1], Y[1], nll[1], grad[1], logml[1], what="fit 1 (after the ladder) ")
    for b in (0, 2):
        close(0, th[b], X[b], Y[b], nll[b], grad[b], logml[b])
    good = ctx.multi_nll_grad_batch(Xgood, Ygood, thgood, 0)   # the same call size without the bad neighbour
    assert good[0] == 0
    for b in (0, 2):
        assert np.array_equal(good[1][b], nll[b]) and np.array_equal(good[2][b], grad[b]) and np.array_equal(good[3][b], logml[b])


def test_fit_that_stays_indefinite_is_nan_neighbours_are_right(engine):
    """Host form: the ladder gives up on fit 1 (negative definite), the call returns its status; device form: no ladder."""
    import torch
    B, N, d, P, kid = 3, 200, 2, 5, 1
    X, Y, theta = problem(B, N, d, P, kid, 9)
    theta[1, -1] = -2.0 * theta[1, 0]
    ctx = ctx_for(engine, B, N, d, P)
    rc, nll, grad, logml, info = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc > 0 and info[1] == rc and info[0] == 0 and info[2] == 0
    assert np.isnan(nll[1]) and np.all(np.isnan(grad[1])) and np.all(np.isnan(logml[1]))
    for b in (0, 2):
        close(kid, theta[b], X[b], Y[b], nll[b], grad[b], logml[b])
    dX, dY, dth = device_arrays(torch, X, Y, theta)
    outs = device_outputs(torch, B, P, theta.shape[1])
    assert ctx.multi_nll_grad_batch_device(B, N, d, P, kid, dX.data_ptr(), dY.data_ptr(), dth.data_ptr(), 0,
                                           *[t.data_ptr() for t in outs[:2]], theta.shape[1], outs[2].data_ptr(),
                                           outs[3].data_ptr()) == 0
    torch.cuda.synchronize()
    dn, dg, dl, di = (t.cpu().numpy() for t in outs)
    assert di[1] > 0 and di[0] == 0 and di[2] == 0
    assert np.isnan(dn[1]) and np.all(np.isnan(dg[1])) and np.all(np.isnan(dl[1]))
    for b in (0, 2):
        assert dn[b] == nll[b] and np.array_equal(dg[b], grad[b]) and np.array_equal(dl[b], logml[b])


# ---- the optimiser -------------------------------------------------------------------------------------------------------
OPT_WINDOWS = [(0, 130, 3), (1, 130, 3), (2, 134, 4), (3, 130, 3), (4, 130, 3)]   # d = 1 on the time base, from all-ones


@pytest.fixture(scope="module")
def opt_runs(engine):
    """One engine optimisation and one scipy optimisation of the oracle per window; shared, never modified."""
    runs = {}
    for kid, N, P in OPT_WINDOWS:
        X, Y = window(N, 1, P, 40 + kid)
        ctx = ctx_for(engine, 2, N, 1, P, max_m=N)
        th, lml, nev = ctx.optimize_multi_batch(X[None], Y[None], kid, np.ones(moo.n_theta(kid, 1)))
        runs[kid] = (X, Y, ctx, th[0], lml[0], nev[0], moo.optimize_multi(kid, X, Y))
    return runs


@pytest.mark.parametrize("kid,N,P", OPT_WINDOWS)
def test_optimum_is_the_oracles(opt_runs, kid, N, P):
    X, Y, ctx, th, lml, nev, (oth, olml, onev, warn) = opt_runs[kid]
    print(f"kid {kid}: engine {nev} evaluations, scipy {onev}; sum logml {lml:.9g} against {olml:.9g}; theta {th} against {oth}")
    assert warn == 0 and nev <= 1000 and np.all(th > 0)
    assert lml >= olml - 1e-6 * abs(olml)
    assert lml == pytest.approx(-moo.nll_and_grad_multi(kid, th, X, Y)[0], rel=1e-8)   # the value reported is the value at theta
    np.testing.assert_allclose(th, oth, rtol=1e-4)
    # the fit at the optimum, through the fixed-theta call
    Xs = X[-1, 0] + 1.0 + np.arange(7.0)[:, None]
    rc, mean, var, logml, info = ctx.fit_predict_multi_batch(X[None], Y[None], Xs[None], th[None], kid)
    assert rc == 0 and not info.any()
    assert max(errors(mean[0], var[0], logml[0], *fit_predict_multi(kid, th, X, Y, Xs))) <= TOL


@pytest.mark.parametrize("kid", [1, 2])
def test_optimize_batch_of_two_matches_each_alone(engine, opt_runs, kid):
    N, P = {1: (130, 3), 2: (134, 4)}[kid]
    X, Y, ctx, th, lml, nev, _ = opt_runs[kid]
    X2, Y2 = window(N, 1, P, 77 + kid, tick0=19)
    thb, lmlb, nevb = ctx.optimize_multi_batch(np.stack([X, X2]), np.stack([Y, Y2]), kid, np.ones(len(th)))
    th2, lml2, _ = ctx.optimize_multi_batch(X2[None], Y2[None], kid, np.ones(len(th)))
    print(f"kid {kid}: evaluations {nevb} in the batch, {nev} alone")
    for b, (t1, l1) in enumerate(((th, lml), (th2[0], lml2[0]))):
        assert lmlb[b] == pytest.approx(l1, rel=1e-9) and nevb[b] <= 1000
        np.testing.assert_allclose(thb[b], t1, rtol=1e-6)


def test_optimize_climbs_the_jitter_ladder(engine):
    """test_gpu_optimize.py::test_optimize_batch_climbs_the_jitter_ladder's start with P = 2: window 1 has duplicated inputs
    and starts at amplitude 1e9 with (almost) no noise."""
    N = 96
    rng = np.random.default_rng(77)
    xa = np.sort(rng.normal(size=N))
    xb = np.repeat(np.sort(rng.normal(size=N // 2)), 2)
    X = np.stack([xa, xb])[:, :, None]
    Y = np.stack([np.sin(2.0 * X[:, :, 0]), np.cos(X[:, :, 0])], axis=1) + 0.01 * rng.normal(size=(2, 2, N))
    Y[1] = np.repeat(Y[1][:, ::2], 2, axis=1)
    th0 = np.array([[1.0, 1.0, 1.0], [1e9, 1.0, 1e-10]])
    ctx = ctx_for(engine, 2, N, 1, 2)
    rc, nll0, _, _, info0 = ctx.multi_nll_grad_batch(X, Y, th0, 0)
    assert rc == 0 and np.all(np.isfinite(nll0))
    th, lml, nev = ctx.optimize_multi_batch(X, Y, 0, th0.copy(), max_evals=60)
    print("evaluations", nev, "sum logml", lml, "theta", th)
    assert np.all(np.isfinite(lml)) and np.all(np.isfinite(th)) and np.all(th > 0)
    assert np.all(lml >= -nll0)


# ---- errors and state --------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=16, max_d=1, max_batch=2)
    buf = np.ones(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 8, 1, 2, 2)   # batch, N, d, P, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, th=p, stride=4, nll=p, grad=p, gstride=4):
        return lib.cgp_multi_nll_grad_batch(h, *shape, x, y, th, stride, nll, grad, gstride, p, ip)

    def dev(h=ctx.h, shape=shape, x=a, y=a, th=a, nll=a, grad=a, gstride=4, info=a):
        return lib.cgp_multi_nll_grad_batch_device(h, *shape, x, y, th, None, nll, grad, gstride, None, info, None)

    def opt(h=ctx.h, shape=shape, x=p, y=p, th=p, stride=4):
        return lib.cgp_optimize_multi_batch(h, *shape, x, y, th, stride, 5, None, None)

    calls = (host, dev, opt)
    assert all(f() == ESTATE for f in calls)                                      # no reservation at all
    # the order of the answers: no context and P = 0 before the missing reservation ...
    assert all(f(h=None) == EINVAL and f(shape=(1, 9, 1, 0, 2)) == EINVAL for f in calls) and lib.cgp_multi_grad_reserve(None, 1, 2) == EINVAL
    assert lib.cgp_multi_grad_reserve(ctx.h, 1, 2) == ESTATE                      # needs cgp_multi_reserve first
    assert lib.cgp_multi_reserve(ctx.h, 1, 2) == 0
    assert all(f() == ESTATE for f in calls)                                      # ... and the A scratch
    assert all(f(shape=(2, 9, 1, 1, 2)) == ESTATE for f in calls)                 # ... a missing reservation before a small one
    for mb, mp in ((0, 2), (3, 2), (1, 0), (1, 4097)):
        assert lib.cgp_multi_grad_reserve(ctx.h, mb, mp) == EINVAL
    assert lib.cgp_multi_grad_reserve(ctx.h, 2, 2) == ESTATE and lib.cgp_multi_grad_reserve(ctx.h, 1, 3) == ESTATE   # not covered
    assert all(f() == ESTATE for f in calls)                                      # a refused reservation leaves none
    assert lib.cgp_multi_grad_reserve(ctx.h, 1, 2) == 0
    for s in ((1, 8, 1, 3, 2), (2, 8, 1, 2, 2)):                                  # P, batch beyond the reservation
        assert all(f(shape=s) == ECAPACITY for f in calls)
    for s in ((2, 9, 1, 1, 2), (1, 9, 1, 3, 2), (2, 9, 1, 1, 5)):                 # ... the capacity before the arrays and the kernel id
        assert all(f(shape=s, x=None) == ECAPACITY for f in calls)
    assert all(f(shape=(1, 8, 1, 0, 2)) == EINVAL for f in calls)                 # P = 0
    assert all(f(shape=(1, 8, 1, 2, 5)) == EINVAL for f in calls)                 # kernel id
    assert all(f(shape=(1, 17, 1, 2, 2)) == ECAPACITY for f in calls)             # N beyond the context
    for f in calls:
        assert f(x=None) == EINVAL and f(y=None) == EINVAL and f(th=None) == EINVAL
    assert host(nll=None) == EINVAL and host(grad=None) == EINVAL and host(stride=3) == EINVAL and host(gstride=3) == EINVAL
    assert dev(nll=None) == EINVAL and dev(grad=None) == EINVAL and dev(gstride=3) == EINVAL and dev(info=None) == EINVAL
    assert opt(stride=3) == EINVAL
    bad = np.ones(8)
    bad[2] = 0.0
    assert opt(th=engine._p(bad)) == EINVAL                                       # theta <= 0
    small_m = engine.Context(max_n=16, max_m=4, max_d=1, max_batch=1)             # max_m >= N, as every gradient call
    assert lib.cgp_multi_reserve(small_m.h, 1, 2) == 0 and lib.cgp_multi_grad_reserve(small_m.h, 1, 2) == 0
    assert all(f(h=small_m.h) == ECAPACITY for f in calls)
    f32 = engine.Context(max_n=16, max_m=16, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_multi_grad_reserve(f32.h, 1, 2) == EINVAL and all(f(h=f32.h) == EINVAL for f in calls)
    # both contexts are still usable
    X, Y, theta = problem(1, 8, 1, 2, 2, 1)
    Xs = X[:, -1:, :] + 1.0
    for c, tol in ((ctx, 1e-6), (f32, 1e-3)):
        rc, mean, var, _, _ = c.fit_predict_batch(X, Y[:, 0], Xs, theta, 2)
        omu, _ = go.predict(go.fit(2, theta[0], X[0], Y[0, 0]), Xs[0])
        assert rc == 0 and np.max(np.abs(mean[0] - omu)) <= tol * np.max(np.abs(omu))
    rc, nll, grad, logml, _ = ctx.multi_nll_grad_batch(X, Y, theta, 2)
    assert rc == 0
    close(2, theta[0], X[0], Y[0], nll[0], grad[0], logml[0])
    assert ctx.multi_reserve(2, 5) == 0 and ctx.multi_grad_reserve(2, 5) == 0     # second reservations replace the first
    X, Y, theta = problem(2, 8, 1, 5, 2, 2)
    rc, nll, grad, logml, _ = ctx.multi_nll_grad_batch(X, Y, theta, 2)
    assert rc == 0
    close(2, theta[1], X[1], Y[1], nll[1], grad[1], logml[1])
    assert ctx.multi_reserve(1, 2) == 0                                           # cgp_multi_reserve again, smaller: a call must fit both
    assert lib.cgp_multi_nll_grad_batch(ctx.h, 2, 8, 1, 5, 2, engine._p(X), engine._p(Y), engine._p(theta), 4, p, p, 4, None,
                                        None) == ECAPACITY


def test_the_calls_leave_other_contexts_alone(engine):
    """A cgp_fit + cgp_predict pair on another context of the process: the same bits before and after the calls of this section."""
    N, d, P, kid = 200, 2, 6, 1
    X, Y, theta = problem(2, N, d, P, kid, 3)
    Xs = X[0][-40:] + 0.1
    other = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=1)

    def pair():
        assert other.fit(X[0], Y[0, 0], kid, theta[0])[0] == 0
        return other.predict(Xs)

    before = pair()
    ctx = ctx_for(engine, 2, N, d, P)
    rc, nll, grad, logml, _ = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    assert rc == 0
    th, lml, nev = ctx.optimize_multi_batch(X, Y, kid, theta, max_evals=3)
    resident = other.predict(Xs)      # the fit that was resident while the other context worked
    after = pair()
    for a, b, c in zip(before, resident, after):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    close(kid, theta[0], X[0], Y[0], nll[0], grad[0], logml[0])
    assert np.all(lml >= -nll)


def test_symbols_present(engine):
    for name in ("cgp_multi_grad_reserve", "cgp_multi_nll_grad_batch", "cgp_multi_nll_grad_batch_device", "cgp_optimize_multi_batch"):
        assert name in engine.EXPORTS and hasattr(engine.load(), name)
