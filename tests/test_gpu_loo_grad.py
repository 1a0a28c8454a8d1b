"""GPU tests of the leave-one-out objective (cgp_loo_grad_reserve, cgp_loo_nll_grad, cgp_loo_nll_grad_batch[_device],
cgp_optimize_loo_batch: value, gradient and optimiser of nlpd = -lpd_sum) against tests/loo_grad_oracle.py, through engine.py.
Bars are the project's: 1e-6 for nlpd (relative) and for the gradient against max|grad| (test_gpu_multi_opt.py::close); SURVEY 8c
for optima; bitwise wherever the header promises it.  Every window compared with the oracle is one of tests/loo_grad_cases.py's,
which tests/test_oracle_loo_grad.py holds to: no jitter, oracle within 1e-8 of max|grad| of its central difference."""
import numpy as np
import pytest

from conftest import load_golden
import loo_oracle as lo
import loo_grad_oracle as lgo
import loo_grad_cases as lc

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def ctx_for(engine, B, N, d, max_n=None):
    ctx = engine.Context(max_n=max_n or N, max_m=max_n or N, max_d=d, max_batch=B)
    assert ctx.loo_grad_reserve(B) == 0
    return ctx


def close(kid, theta, X, y, nlpd, grad, tol=TOL, what=""):
    onlpd, og, _, jit = lgo.nlpd_and_grad(kid, theta, X, y)
    en = abs(nlpd - onlpd) / abs(onlpd)
    eg = np.max(np.abs(grad - og)) / np.max(np.abs(og))
    print(f"{what}errors / bar: nlpd {en / tol:.3g} grad {eg / tol:.3g}")
    assert jit == 0.0 and en <= tol and eg <= tol, (en, eg)


@pytest.mark.parametrize("kid,d", lc.KERNEL_SHAPES)
def test_every_kernel(engine, kid, d):
    X, y, theta = lc.kernel_problem(kid, d)
    ctx = ctx_for(engine, 2, 130, d)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, theta, kid)
    assert rc == 0 and not info.any()
    for b in range(2):
        close(kid, theta[b], X[b], y[b], nlpd[b], grad[b], what=f"fit {b}: ")


@pytest.mark.parametrize("d", lc.EDGE_D)
@pytest.mark.parametrize("N", lc.EDGE_N)
def test_tile_edges(engine, N, d):
    """One tile, the tile edge, and three block steps with a one-row last tile: at N = 257 the dense inner dimension crosses a
    tile that is neither the pair's row tile nor its column tile, and the transposed store lands in a third tile row."""
    kid = lc.edge_kernel(N, d)
    X, y, theta = lc.edge_problem(N, d)
    ctx = ctx_for(engine, 2, N, d)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, theta, kid)
    assert rc == 0 and not info.any() and grad.shape == (2, lgo.n_theta(kid, d))
    for b in range(2):
        close(kid, theta[b], X[b], y[b], nlpd[b], grad[b], what=f"fit {b}: ")


@pytest.fixture(scope="module")
def schedule_runs(engine):
    """One call per schedule; fit 1's window also sits in the last slot.  Shared by the tests below, never modified."""
    runs = {}
    for B, N in lc.SCHEDULES:
        X, y, theta = lc.schedule_problem(B, N)
        ctx = ctx_for(engine, B, N, 3)
        out = ctx.loo_nll_grad_batch(X, y, theta, 1)
        # the same call size with every other window replaced: new neighbours, other slot for the window of fit 1
        X2, y2, theta2 = lc.problem(B, N, 3, 1, 1007 + B)
        X2[0], y2[0], theta2[0] = X[1], y[1], theta[1]
        out2 = ctx.loo_nll_grad_batch(X2, y2, theta2, 1)
        runs[B] = (X, y, theta, out, out2)
        ctx.close()
    return runs


@pytest.mark.parametrize("B,N", lc.SCHEDULES)
def test_every_schedule_meets_the_oracle(schedule_runs, B, N):
    X, y, theta, (rc, nlpd, grad, logml, info), _ = schedule_runs[B]
    assert rc == 0 and not info.any()
    for b in lc.schedule_checked(B):
        close(1, theta[b], X[b], y[b], nlpd[b], grad[b], what=f"fit {b}: ")
    assert np.all(np.isfinite(nlpd)) and np.all(np.isfinite(grad))


@pytest.mark.parametrize("B,N", lc.SCHEDULES)
def test_outputs_do_not_depend_on_slot_or_neighbours(schedule_runs, B, N):
    _, _, _, out, out2 = schedule_runs[B]
    for u, w in zip(out[1:4], out2[1:4]):
        assert np.array_equal(u[1], u[B - 1]) and np.array_equal(u[1], w[0])


@pytest.mark.parametrize("src,pin", [("mp_rbfbrownian_n134", "loo_grad_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_grad_mp_m32_n134"),
                                     ("matern_mp_m52_n134", "loo_grad_mp_m52_n134")])
def test_mpmath_pins(engine, src, pin):
    """The 50-digit values themselves, not the float64 oracle."""
    g, p = load_golden(src), load_golden(pin)
    X, y, theta, kid = g["X"], g["y"], g["theta"], int(g["kernel_id"])
    ctx = ctx_for(engine, 1, len(y), 1)
    nlpd, grad = ctx.loo_nll_grad(X, y, kid, theta)
    en, eg = abs(nlpd - float(p["nlpd"])) / abs(float(p["nlpd"])), np.max(np.abs(grad - p["grad"])) / np.max(np.abs(p["grad"]))
    print(f"errors / bar: nlpd {en / TOL:.3g} grad {eg / TOL:.3g}")
    assert en <= TOL and eg <= TOL


@pytest.mark.parametrize("B,N,d,kid", [(1, 257, 3, 3), (4, 200, 2, 1), (30, 130, 1, 2)])
def test_nlpd_is_lpd_sum_negated_and_logml_is_loo_batchs(engine, B, N, d, kid):
    X, y, theta = lc.problem(B, N, d, kid, 12 + B)
    ctx = ctx_for(engine, B, N, d)
    loo = ctx.loo_batch(X, y, theta, kid)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, theta, kid)
    assert rc == 0 and loo[0] == 0
    assert np.array_equal(nlpd, -loo[4]) and np.array_equal(logml, loo[5])


def test_single_call_is_the_batch_of_one_and_leaves_the_context_fitted(engine):
    N, d, kid = 257, 3, 3
    X, y, theta = lc.problem(1, N, d, kid, 5)
    ctx = ctx_for(engine, 1, N, d)
    rc, nlpd, grad, _, _ = ctx.loo_nll_grad_batch(X, y, theta, kid)
    n1, g1 = ctx.loo_nll_grad(X[0], y[0], kid, theta[0])
    assert rc == 0 and n1 == nlpd[0] and np.array_equal(g1, grad[0])
    Xs = X[0][-20:] + 0.1
    pm, pv = ctx.predict(Xs)
    om, ov = lo.mo.predict(lo.mo.fit(kid, theta[0], X[0], y[0]), Xs)
    assert np.max(np.abs(pm - om)) <= TOL * np.max(np.abs(om)) and np.max(np.abs(pv - ov) / ov) <= TOL


def device_arrays(torch, X, y, theta):
    th = np.zeros((X.shape[0], 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, th)]


@pytest.mark.parametrize("B,N", [(3, 130), (50, 257)])
def test_host_device_and_graph_replay_agree_bitwise(engine, B, N):
    """The legacy stream, CGP_STREAM_CTX and a captured side stream against the host form."""
    import torch
    d, kid = 3, 1
    nth = d + 2
    X, y, theta = lc.problem(B, N, d, kid, 9 + B)
    ctx = ctx_for(engine, B, N, d)
    host = ctx.loo_nll_grad_batch(X, y, theta, kid)
    assert host[0] == 0
    dX, dy, dth = device_arrays(torch, X, y, theta)
    f = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    outs = [f(B), f(B, nth), f(B)]
    dinfo = torch.empty(B, dtype=torch.int32, device="cuda")

    def clear():
        for t in outs:
            t.fill_(-1.0)
        dinfo.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        for t, h in zip(outs, host[1:4]):
            assert np.array_equal(t.cpu().numpy(), h)
        assert not dinfo.cpu().numpy().any()

    def enqueue(s):
        assert ctx.loo_nll_grad_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, outs[0].data_ptr(),
                                             outs[1].data_ptr(), nth, outs[2].data_ptr(), dinfo.data_ptr(), stream=s) == 0

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


def test_a_smaller_fit_sees_nothing_of_the_scratch_of_a_larger_one(engine):
    """N = 256 fills both tiles of the scratch; N = 130 in the same context then reads rows and columns 130 .. 255 of it in its
    dense inner loop: they must have been stored as zeros, whatever the factor panel holds there."""
    d, kid = 3, 1
    Xl, yl, thl = lc.problem(2, 256, d, kid, 31)
    Xs, ys, ths = lc.problem(2, 130, d, kid, 32)
    used = ctx_for(engine, 2, 256, d)
    assert used.loo_nll_grad_batch(Xl, yl, thl, kid)[0] == 0
    got = used.loo_nll_grad_batch(Xs, ys, ths, kid)
    fresh = ctx_for(engine, 2, 130, d, max_n=256).loo_nll_grad_batch(Xs, ys, ths, kid)
    assert got[0] == 0 and fresh[0] == 0
    for u, w in zip(got[1:4], fresh[1:4]):
        assert np.array_equal(u, w)
    for b in range(2):
        close(kid, ths[b], Xs[b], ys[b], got[1][b], got[2][b], what=f"fit {b}: ")


def ladder_problem():
    """test_gpu_loo.py::test_jitter_ladder_is_per_fit's input: fit 1 needs the first rung."""
    rng = np.random.default_rng(21)
    N, d, B = 200, 1, 3
    X = np.stack([np.sort(rng.normal(size=(N, d)), 0) for _ in range(B)])
    Xgood = X.copy()
    X[1, :, 0] = np.repeat(np.arange(N // 2, dtype=float), 2)         # duplicated inputs -> rank deficient K
    y, ygood = np.sin(X[:, :, 0]), np.sin(Xgood[:, :, 0])
    th = np.array([[1.0, 1.0, 0.05], [1.0, 3.0, -1e-8 - 2e-7], [1.0, 1.0, 0.05]])   # window 1: slightly indefinite
    thgood = np.array([[1.0, 1.0, 0.05]] * 3)
    return X, y, th, Xgood, ygood, thgood


def test_jitter_ladder_is_per_fit(engine):
    """Fit 1 is re-submitted as a call of one fit in slab 0 and ends at the oracle's jitter; its nlpd is cgp_loo_batch's lpd_sum
    (which test_gpu_loo.py holds to the oracle at that jitter) negated; fits 0 and 2 are bitwise what they are without it."""
    X, y, th, Xgood, ygood, thgood = ladder_problem()
    want = lo.loo(0, th[1], X[1], y[1])
    assert want.jitter > 0
    ctx = ctx_for(engine, 3, 200, 1)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, th, 0)
    assert rc == 0 and not info.any() and np.all(np.isfinite(grad)) and np.all(np.isfinite(nlpd))
    assert np.array_equal(nlpd, -ctx.loo_batch(X, y, th, 0)[4])
    for b in (0, 2):
        close(0, th[b], X[b], y[b], nlpd[b], grad[b], what=f"fit {b}: ")
    good = ctx.loo_nll_grad_batch(Xgood, ygood, thgood, 0)
    assert good[0] == 0
    for b in (0, 2):
        assert nlpd[b] == good[1][b] and np.array_equal(grad[b], good[2][b]) and logml[b] == good[3][b]
    # the single call climbs the same ladder and reports the jitter
    n1, g1 = ctx.loo_nll_grad(X[1], y[1], 0, th[1])
    assert n1 == nlpd[1] and np.array_equal(g1, grad[1])
    assert abs(ctx.last_jitter() - want.jitter) <= 1e-12 * want.jitter


def test_fit_that_stays_indefinite_is_nan_neighbours_are_right(engine):
    """Host form: the ladder gives up on fit 1 (negative definite), the call returns its status; device form: no ladder."""
    import torch
    B, N, d, kid = 3, 200, 2, 1
    X, y, theta = lc.problem(B, N, d, kid, 8)
    good = theta.copy()
    theta[1, -1] = -2.0 * theta[1, 0]
    ctx = ctx_for(engine, B, N, d)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, theta, kid)
    assert rc > 0 and info[1] == rc and info[0] == 0 and info[2] == 0
    assert np.isnan(nlpd[1]) and np.all(np.isnan(grad[1]))
    ref = ctx.loo_nll_grad_batch(X, y, good, kid)
    for b in (0, 2):
        assert nlpd[b] == ref[1][b] and np.array_equal(grad[b], ref[2][b])
    with pytest.raises(engine.CgpError):
        ctx.loo_nll_grad(X[1], y[1], kid, theta[1])
    with pytest.raises(engine.CgpError):
        ctx.predict(X[1][:3])   # not fitted
    dX, dy, dth = device_arrays(torch, X, y, theta)
    dn, dg = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, 4, dtype=torch.float64, device="cuda")
    di = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert ctx.loo_nll_grad_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, dn.data_ptr(), dg.data_ptr(), 4,
                                         0, di.data_ptr()) == 0
    torch.cuda.synchronize()
    dn, dg, di = dn.cpu().numpy(), dg.cpu().numpy(), di.cpu().numpy()
    assert di[1] > 0 and di[0] == 0 and di[2] == 0 and np.isnan(dn[1]) and np.all(np.isnan(dg[1]))
    for b in (0, 2):
        assert dn[b] == nlpd[b] and np.array_equal(dg[b], grad[b])


def test_argument_state_and_capacity_errors(engine):
    buf = np.zeros(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    ctx = engine.Context(max_n=16, max_m=16, max_d=1, max_batch=2)
    lib = ctx.lib

    def one(h=ctx.h, X=p, N=8, d=1, kid=2, th=p, nl=p, g=p):
        return lib.cgp_loo_nll_grad(h, X, p, N, d, kid, th, nl, g)

    def bat(h=ctx.h, B=1, N=8, d=1, kid=2, X=p, stride=4, nl=p, g=p, gs=4):
        return lib.cgp_loo_nll_grad_batch(h, B, N, d, kid, X, p, p, stride, nl, g, gs, p, ip)

    def dev(h=ctx.h, B=1, N=8, d=1, kid=2, X=a, nl=a, g=a, gs=4, info=a):
        return lib.cgp_loo_nll_grad_batch_device(h, B, N, d, kid, X, a, a, None, nl, g, gs, a, info, None)

    def opt(h=ctx.h, B=1, N=8, d=1, kid=2, X=p, th=p, stride=4):
        return lib.cgp_optimize_loo_batch(h, B, N, d, kid, X, p, th, stride, 5, None, None, None)

    for f in (one, bat, dev, opt):
        assert f() == ESTATE   # no reservation
    assert lib.cgp_loo_grad_reserve(None, 1) == EINVAL and lib.cgp_loo_grad_reserve(ctx.h, 0) == EINVAL
    assert lib.cgp_loo_grad_reserve(ctx.h, 3) == EINVAL   # beyond the context's max_batch
    assert ctx.loo_grad_reserve(1) == 0
    for f in (bat, dev, opt):
        assert f(B=2) == ECAPACITY   # batch above the reservation
    assert ctx.loo_grad_reserve(2) == 0
    for f in (one, bat, dev, opt):
        assert f(h=None) == EINVAL
        assert f(N=0) == EINVAL and f(d=0) == EINVAL and f(kid=5) == EINVAL and f(kid=-1) == EINVAL
        assert f(kid=2, d=2) == EINVAL   # RBF x Brownian is one-dimensional
        assert f(N=17) == ECAPACITY and f(kid=1, d=2) == ECAPACITY
        assert f(X=None) == EINVAL
    for f in (one, bat, dev):
        assert f(nl=None) == EINVAL and f(g=None) == EINVAL
    assert bat(B=0) == EINVAL and dev(B=0) == EINVAL and opt(B=0) == EINVAL and bat(B=3) == ECAPACITY and dev(B=3) == ECAPACITY
    assert bat(stride=3) == EINVAL and bat(gs=3) == EINVAL and dev(gs=3) == EINVAL and opt(stride=3) == EINVAL
    assert one(th=None) == EINVAL and dev(info=None) == EINVAL
    assert opt(th=p) == EINVAL   # theta of zeros: not positive
    small_m = engine.Context(max_n=16, max_m=4, max_d=1, max_batch=1)   # needs max_m >= N, as cgp_loo does
    assert small_m.loo_grad_reserve(1) == 0
    assert one(h=small_m.h) == ECAPACITY and bat(h=small_m.h) == ECAPACITY and dev(h=small_m.h) == ECAPACITY
    # the context is still usable
    X, y, theta = lc.problem(1, 8, 1, 2, 1)
    assert np.isfinite(ctx.loo_nll_grad(X[0], y[0], 2, theta[0])[0])


def test_fp32_contexts_are_refused_and_stay_usable(engine):
    ctx = engine.Context(max_n=64, max_m=64, max_d=2, max_batch=2, dtype=F32)
    X, y, theta = lc.problem(2, 64, 2, 1, 4)
    p = engine._p
    buf = np.zeros(2 * 64)
    a = buf.ctypes.data
    lib = ctx.lib
    assert lib.cgp_loo_grad_reserve(ctx.h, 2) == EINVAL
    assert lib.cgp_loo_nll_grad(ctx.h, p(X[0]), p(y[0]), 64, 2, 1, p(theta[0]), p(buf), p(buf)) == EINVAL
    assert lib.cgp_loo_nll_grad_batch(ctx.h, 2, 64, 2, 1, p(X), p(y), p(theta), 4, p(buf), p(buf), 4, None, None) == EINVAL
    assert lib.cgp_loo_nll_grad_batch_device(ctx.h, 2, 64, 2, 1, a, a, a, None, a, a, 4, a, a, None) == EINVAL
    assert lib.cgp_optimize_loo_batch(ctx.h, 2, 64, 2, 1, p(X), p(y), p(theta.copy()), 4, 5, None, None, None) == EINVAL
    rc, logml = ctx.fit(X[0], y[0], 1, theta[0])
    assert rc == 0 and np.isfinite(logml)


def test_symbols_present(engine):
    lib = engine.load()
    for name in ("cgp_loo_grad_reserve", "cgp_loo_nll_grad", "cgp_loo_nll_grad_batch", "cgp_loo_nll_grad_batch_device",
                 "cgp_optimize_loo_batch"):
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert lib.cgp_abi_version() == 3


# ---- the optimiser -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opt_runs(engine):
    """One engine optimisation and one scipy optimisation of the oracle per window; shared, never modified."""
    runs = {}
    for kid, N, seed, _ in lc.OPT_WINDOWS:
        X, y = lc.window(N, 1, seed)
        ctx = ctx_for(engine, 2, N, 1)
        th, lpd, logml, nev = ctx.optimize_loo_batch(X[None], y[None], kid, np.ones(lgo.n_theta(kid, 1)))
        runs[kid] = (X, y, ctx, th[0], lpd[0], logml[0], nev[0], lgo.optimize_loo(kid, X, y))
    return runs


@pytest.mark.parametrize("kid,N,seed,theta_compared", lc.OPT_WINDOWS)
def test_optimum_is_the_oracles(opt_runs, kid, N, seed, theta_compared):
    X, y, ctx, th, lpd, logml, nev, (oth, olpd, onev, warn) = opt_runs[kid]
    print(f"kid {kid}: engine {nev} evaluations, scipy {onev}; lpd_sum {lpd:.9g} against {olpd:.9g}; theta {th} against {oth}")
    assert warn == 0 and nev <= 1000 and np.all(th > 0)
    assert lpd >= olpd - 1e-6 * abs(olpd)
    onl, _, olml, _ = lgo.nlpd_and_grad(kid, th, X, y)
    assert lpd == pytest.approx(-onl, rel=1e-8) and logml == pytest.approx(olml, rel=1e-8)   # the values reported are those at theta
    if theta_compared:
        np.testing.assert_allclose(th, oth, rtol=1e-4)


@pytest.mark.parametrize("kid", [1, 2])
def test_optimize_batch_of_two_matches_each_alone(engine, opt_runs, kid):
    X, y, ctx, th, lpd, _, nev, _ = opt_runs[kid]
    X2, y2 = lc.window(len(y), 1, 77 + kid, tick0=19)
    thb, lpdb, _, nevb = ctx.optimize_loo_batch(np.stack([X, X2]), np.stack([y, y2]), kid, np.ones(len(th)))
    th2, lpd2, _, _ = ctx.optimize_loo_batch(X2[None], y2[None], kid, np.ones(len(th)))
    print(f"kid {kid}: evaluations {nevb} in the batch, {nev} alone")
    for b, (t1, l1) in enumerate(((th, lpd), (th2[0], lpd2[0]))):
        assert lpdb[b] == pytest.approx(l1, rel=1e-9) and nevb[b] <= 1000
        np.testing.assert_allclose(thb[b], t1, rtol=1e-6)


def test_optimize_climbs_the_jitter_ladder(engine):
    """test_gpu_multi_opt.py::test_optimize_climbs_the_jitter_ladder's start on column 0: window 1 has duplicated inputs and
    starts at amplitude 1e9 with (almost) no noise."""
    N = 96
    rng = np.random.default_rng(77)
    xa = np.sort(rng.normal(size=N))
    xb = np.repeat(np.sort(rng.normal(size=N // 2)), 2)
    X = np.stack([xa, xb])[:, :, None]
    Y = np.stack([np.sin(2.0 * X[:, :, 0]), np.cos(X[:, :, 0])], axis=1) + 0.01 * rng.normal(size=(2, 2, N))
    Y[1] = np.repeat(Y[1][:, ::2], 2, axis=1)
    y = np.ascontiguousarray(Y[:, 0])
    th0 = np.array([[1.0, 1.0, 1.0], [1e9, 1.0, 1e-10]])
    ctx = ctx_for(engine, 2, N, 1)
    rc, nl0, _, _, info0 = ctx.loo_nll_grad_batch(X, y, th0, 0)
    assert rc == 0 and np.all(np.isfinite(nl0))
    th, lpd, logml, nev = ctx.optimize_loo_batch(X, y, 0, th0.copy(), max_evals=60)
    print("evaluations", nev, "lpd_sum", lpd, "theta", th)
    assert np.all(np.isfinite(lpd)) and np.all(np.isfinite(th)) and np.all(th > 0)
    assert np.all(lpd >= -nl0)
