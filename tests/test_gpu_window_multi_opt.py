"""GPU tests of the multi-target windows' summed objective (cgp_window_multi_grad_reserve, cgp_window_multi_nll_grad[_device],
cgp_window_optimize_multi).  Parity against the refit oracle tests/window_multi_opt_oracle.py at the project's fp64 bar, 1e-6, in
test_gpu_window_adapt.py's metrics (nll against max(|nll|, 1), the gradient against its largest entry) and logml as
tests/window_multi_oracle.py::errors measures it; routes at 1e-9; the forms bitwise.  No case is skipped:
tests/test_oracle_window_multi_opt.py asserts on the CPU that no window compared here needs jitter.  The largest errors are
printed; DESIGN.md section 9i records them."""
import numpy as np
import pytest

import adapt_oracle as ao
import window_multi_opt_oracle as wmo
import window_multi_oracle as wm
import test_gpu_window_paths as paths

pytestmark = pytest.mark.gpu
TOL = 1e-6
ROUTE = 1e-9
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h
WORST = {"nll": 0.0, "grad": 0.0, "logml": 0.0}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def new_ctx(engine, W, N, d, kid, theta, P, grad=True):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    if P:
        ctx.window_multi_reserve(P)
        if grad:
            ctx.window_multi_grad_reserve()
    return ctx


def streams(W, T, d, P, seed):
    Xw, Yw = zip(*[wm.stream(T, d, P, seed + 17 * w) for w in range(W)])
    return np.stack(Xw), np.stack(Yw)


def errors(nll, g, logml, onll, og, ologml):
    return (abs(nll - onll) / max(abs(onll), 1.0), np.max(np.abs(g - og)) / np.max(np.abs(og)),
            np.max(np.abs(logml - ologml) / np.maximum(1.0, np.abs(ologml))))


def close(nll, g, logml, kid, theta, N, X, Y, t=None, what=""):
    """One window against the oracle's refit of the stream's last min(t, N) samples."""
    assert wmo.jitter(kid, theta, N, X, Y, t) == 0.0, what
    en, eg, el = errors(nll, g, logml, *wmo.nll_and_grad_multi(kid, theta, N, X, Y, t))
    for k, e in (("nll", en), ("grad", eg), ("logml", el)):
        WORST[k] = max(WORST[k], e)
    assert en <= TOL and eg <= TOL and el <= TOL, (what, en, eg, el)
    return en, eg, el


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def parity(engine, kid, N, d, P):
    X, Y, theta = wmo.parity_streams(kid, N, d, P)
    W = wmo.PARITY_W
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    fed, worst = 0, np.zeros(3)
    for t in wmo.parity_ticks(N):
        ctx.window_push_multi(X[:, fed:t], Y[:, fed:t])
        fed = t
        assert ctx.window_state(W - 1) == (min(N, t), 0)
        nll, g, logml = ctx.window_multi_nll_grad()
        assert nll.shape == (W,) and g.shape == (W, len(theta)) and logml.shape == (W, P)
        for w in range(W):
            worst = np.maximum(worst, close(nll[w], g[w], logml[w], kid, theta, N, X[w], Y[w], t, what=f"t {t} w {w}"))
    print(f"kid {kid} N {N} d {d} P {P}: worst errors / bar: nll {worst[0] / TOL:.3g} grad {worst[1] / TOL:.3g} logml {worst[2] / TOL:.3g};"
          f" so far {WORST}")


@pytest.mark.parametrize("P", wmo.PARITY_P)
@pytest.mark.parametrize("kid,N,d", wmo.PARITY)
def test_value_and_gradient_match_the_refit_oracle_over_the_rings_states(engine, kid, N, d, P):
    """Three windows fed uneven pushes; compared after the ticks that leave n = 1, 15, 16, 17, while filling, when just full,
    either side of the ring's compaction at 2 N and past it."""
    parity(engine, kid, N, d, P)


def test_sixty_four_columns(engine):
    parity(engine, *wmo.PARITY_P64)


def test_the_form_above_512(engine):
    """512 < N <= 1024: k_window_multi_z's sixteen-column form feeds the same A and contraction."""
    N, d, P, T = 700, 3, 3, 1500
    X, Y = wm.stream(T, d, P, N)
    theta = wm.theta_of(1, d)
    ctx = new_ctx(engine, 1, N, d, 1, theta, P)
    ctx.window_push_multi(X[None], Y[None])
    nll, g, logml = ctx.window_multi_nll_grad()
    print("N 700 errors / bar:", np.array(close(nll[0], g[0], logml[0], 1, theta, N, X, Y, what="N 700")) / TOL)


def test_gradient_is_the_derivative_of_set_thetas_summed_value(engine):
    """Central finite differences of -sum_p logml[p] through cgp_window_set_theta + cgp_window_predict_multi: no oracle involved."""
    N, d, P, T = 64, 3, 3, 150
    X, Y = wm.stream(T, d, P, 21)
    theta = wm.theta_of(1, d) * np.array([1.3, 0.8, 1.2, 0.9, 1.5])
    ctx = new_ctx(engine, 1, N, d, 1, wm.theta_of(1, d), P)
    ctx.window_push_multi(X[None], Y[None])
    Xs = X[None, -1:]

    def value(th):
        ctx.window_set_theta(th)
        return -np.sum(ctx.window_predict_multi(Xs)[2])

    ctx.window_set_theta(theta)
    _, g, _ = ctx.window_multi_nll_grad()
    for i in range(len(theta)):
        h = 1e-5 * theta[i]
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = (value(tp) - value(tm)) / (2 * h)
        assert abs(fd - g[0, i]) <= 1e-4 * max(abs(g[0, i]), 1e-3 * np.max(np.abs(g[0]))), (i, fd, g[0, i])


def test_routes_single_target_windows(engine):
    """P = 1 against cgp_window_nll_grad on the same context; P = 3 against the sum over three single-target contexts.  To rounding,
    not bitwise: the resident z is incremental, Z is a fresh solve."""
    W, N, d, kid, T = 3, 48, 2, 1, 131
    X, Y = streams(W, T, d, 3, 40)
    theta = np.stack([wm.theta_of(kid, d) * (1.0 + 0.1 * w) for w in range(W)])
    one = new_ctx(engine, W, N, d, kid, theta, 1)
    one.window_push_multi(X, Y[:, :, :1])
    nll, g, logml = one.window_multi_nll_grad()
    nll1, g1 = one.window_nll_grad()
    assert np.max(np.abs(nll - nll1) / np.maximum(np.abs(nll1), 1.0)) <= ROUTE
    assert max(rel(g[w], g1[w]) for w in range(W)) <= ROUTE
    assert np.array_equal(-logml[:, 0], nll)
    three = new_ctx(engine, W, N, d, kid, theta, 3)
    three.window_push_multi(X, Y)
    nll, g, logml = three.window_multi_nll_grad()
    snll, sg = np.zeros(W), np.zeros((W, d + 2))
    for p in range(3):
        c = new_ctx(engine, W, N, d, kid, theta, 0)
        c.window_push(X, Y[:, :, p])
        a, b = c.window_nll_grad()
        snll, sg = snll + a, sg + b
        assert np.max(np.abs(logml[:, p] + a) / np.maximum(np.abs(a), 1.0)) <= ROUTE
    assert np.max(np.abs(nll - snll) / np.maximum(np.abs(snll), 1.0)) <= ROUTE
    assert max(rel(g[w], sg[w]) for w in range(W)) <= ROUTE


def test_route_the_batch_objective_on_the_downloaded_samples(engine):
    W, N, d, kid, P, T = 3, 64, 3, 1, 5, 150
    X, Y = streams(W, T, d, P, 90)
    theta = np.stack([wm.theta_of(kid, d) * (1.0 + 0.1 * w) for w in range(W)])
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    ctx.window_push_multi(X, Y)
    nll, g, logml = ctx.window_multi_nll_grad()
    b = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
    b.multi_reserve(W, P)
    b.multi_grad_reserve(W, P)
    rc, bnll, bg, blogml, info = b.multi_nll_grad_batch(X[:, -N:], np.ascontiguousarray(Y[:, -N:].transpose(0, 2, 1)), theta, kid)
    assert rc == 0 and not info.any()
    assert np.max(np.abs(nll - bnll) / np.maximum(np.abs(bnll), 1.0)) <= ROUTE
    assert max(rel(g[w], bg[w]) for w in range(W)) <= ROUTE
    assert np.max(np.abs(logml - blogml) / np.maximum(np.abs(blogml), 1.0)) <= ROUTE


def test_host_device_and_graph_replay_agree_bitwise(engine):
    """Also: two calls in a row are identical, and logml = NULL leaves nll and grad identical and writes no logml."""
    import torch
    W, N, d, kid, T, P = 3, 40, 3, 1, 100, 5
    nth, stride = d + 2, d + 4
    X, Y = streams(W, T, d, P, 500)
    ctx = new_ctx(engine, W, N, d, kid, wm.theta_of(kid, d), P)
    ctx.window_push_multi(X, Y)
    ref = ctx.window_multi_nll_grad()
    for a, b in zip(ref, ctx.window_multi_nll_grad()):
        assert np.array_equal(a, b)
    nll, g, none = ctx.window_multi_nll_grad(want_logml=False)
    assert none is None and np.array_equal(nll, ref[0]) and np.array_equal(g, ref[1])
    wide = ctx.window_multi_nll_grad(nth=stride)
    assert np.array_equal(wide[1][:, :nth], ref[1]) and np.all(wide[1][:, nth:] == 0.0)
    out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((W,), (W, stride), (W, P))]

    def clear():
        for t in out:
            t.fill_(-1.0)
        torch.cuda.synchronize()

    def check(n=3):
        ctx.synchronize()
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in out]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1][:, :nth], ref[1]) and np.all(got[1][:, nth:] == -1.0)
        assert np.array_equal(got[2], ref[2]) if n == 3 else np.all(got[2] == -1.0)

    def enqueue(s, logml=True):
        ptrs = [t.data_ptr() for t in out]
        assert ctx.window_multi_nll_grad_device(P, ptrs[0], ptrs[1], stride, ptrs[2] if logml else 0, stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    clear()
    enqueue(0, logml=False)
    check(2)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()


def test_a_window_does_not_depend_on_its_slot_and_columns_permute(engine):
    """Slot 0 of 1 equals slot 4 of 5 with different neighbours, bitwise.  Permuting the columns permutes logml bitwise; nll and the
    gradient move by rounding only (the sum over the columns runs in another order)."""
    N, d, kid, T, P = 40, 2, 1, 57, 17
    X, Y = streams(5, T, d, P, 77)
    theta = wm.theta_of(kid, d)
    perm = np.random.default_rng(5).permutation(P)

    def run(Xc, Yc):
        ctx = new_ctx(engine, len(Xc), N, d, kid, theta, Yc.shape[2])
        for i in range(T):
            ctx.window_push_multi(Xc[:, i:i + 1], Yc[:, i:i + 1])
        return ctx.window_multi_nll_grad()

    nll, g, logml = run(X, Y)
    n1, g1, l1 = run(X[4:], Y[4:])
    assert n1[0] == nll[4] and np.array_equal(g1[0], g[4]) and np.array_equal(l1[0], logml[4])
    pn, pg, pl = run(X, Y[:, :, perm])
    assert np.array_equal(pl, logml[:, perm])
    # the columns' sum in another order: a few ulps of the summed magnitudes; the gradient's rank-P term, which cancels against
    # P Ky^-1, at the project's route bar
    assert np.all(np.abs(pn - nll) <= 1e-13 * np.sum(np.abs(logml), axis=1)) and max(rel(pg[w], g[w]) for w in range(5)) <= ROUTE


def test_the_call_does_not_touch_the_windows(engine):
    """A twin context that made no call gives bitwise the same next push, state words, cgp_window_predict_multi and
    cgp_window_nll_grad."""
    W, N, d, kid, P, T = 2, 48, 2, 1, 3, 170
    X, Y = streams(W, T, d, P, 70)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -30:] + 0.1
    outs = []
    for between in (True, False):
        ctx = new_ctx(engine, W, N, d, kid, theta, P)
        ctx.window_push_multi(X[:, :90], Y[:, :90])
        if between:
            ctx.window_multi_nll_grad()
            ctx.window_multi_nll_grad(want_logml=False)
        o = ctx.window_push_multi(X[:, 90:], Y[:, 90:]) + ctx.window_predict_multi(Xs) + ctx.window_nll_grad() + ctx.window_loo()
        outs.append(o + (np.array([ctx.window_state(w) for w in range(W)]),))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_failed_window_answers_nan_and_is_revived_for_every_column(engine):
    """test_gpu_window_multi.py's failure recipe: the victim answers NaN in nll, the gradient and its P logml entries, the
    neighbours are bitwise what they are beside a healthy one; after a reviving set_theta it meets the oracle for every column."""
    kid, W, N, d, P, victim, pre, T, tl, K = 1, 3, 32, 2, 3, 1, 41, 9, 4, 6
    ts = pre + tl
    X, y, bad, good = paths.failing_streams(kid, W, d, pre + T + K, 31, victim, ts)
    rng = np.random.default_rng(8)
    Y = np.stack([y] + [y * (1.5 + p) + rng.normal(0, 0.02, y.shape) for p in range(1, P)], axis=2)
    others = np.arange(W) != victim
    A, B = new_ctx(engine, W, N, d, kid, bad, P), new_ctx(engine, W, N, d, kid, good, P)
    for c in (A, B):
        c.window_push_multi(X[:, :pre], Y[:, :pre])
    *_, rc = A.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T], check=False)
    B.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T])
    assert rc == tl + 1 and A.window_state(victim) == (N, tl + 1)
    na, ga, la = A.window_multi_nll_grad()
    nb, gb, lb = B.window_multi_nll_grad()
    assert np.isnan(na[victim]) and np.all(np.isnan(ga[victim])) and np.all(np.isnan(la[victim]))
    for a, b in ((na, nb), (ga, gb), (la, lb)):
        assert np.array_equal(a[others], b[others]) and np.all(np.isfinite(a[others]))
    na2, ga2, none = A.window_multi_nll_grad(want_logml=False)
    assert np.array_equal(na2, na, equal_nan=True) and np.array_equal(ga2, ga, equal_nan=True)
    _, info = A.window_set_theta(good, select=~others)
    assert np.all(info == 0) and A.window_state(victim) == (N, 0)
    nll, g, logml = A.window_multi_nll_grad()
    for w in range(W):
        close(nll[w], g[w], logml[w], kid, good[w], N, X[w], Y[w], pre + T, what=f"revived, window {w}")


def test_empty_windows_answer_zero(engine):
    W, N, d, kid, P = 2, 16, 1, 2, 3
    ctx = new_ctx(engine, W, N, d, kid, wm.theta_of(kid, d), P)
    for want in (True, False):
        nll, g, logml = ctx.window_multi_nll_grad(want_logml=want)
        assert np.all(nll == 0.0) and np.all(g == 0.0) and (logml is None or np.all(logml == 0.0))
    X, Y = wm.stream(4, d, P, 1)
    on, og, ol = wmo.nll_and_grad_multi(kid, wm.theta_of(kid, d), N, X, Y, 0)   # the oracle's rule is the same
    assert on == 0.0 and not og.any() and not ol.any()


# ---- cgp_window_optimize_multi ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,N,d,P,T,seed", wmo.OPT_CASES)
def test_optimize_multi_matches_optimize_multi_batch_on_the_same_samples(engine, kid, N, d, P, T, seed):
    """Same optimiser, same start, same samples: the bars of test_window_optimize_matches_optimize_batch_on_the_same_samples.
    Afterwards the forecast of every column meets the refit oracle under the returned theta with no further call, and a push
    meets the oracle's stream for column 0."""
    K = 4
    X, Y = wm.stream(T + K, d, P, seed)
    th0 = wmo.opt_start(kid, d)
    ctx = new_ctx(engine, 1, N, d, kid, th0, P)
    ctx.window_push_multi(X[None, :T], Y[None, :T])
    start = -ctx.window_multi_nll_grad()[0][0]
    th, lml, nev = ctx.window_optimize_multi(max_evals=200)
    assert np.all(th > 0) and 1 < nev[0] <= 200 and lml[0] >= start - 1e-9
    nll, _, _ = ctx.window_multi_nll_grad()
    assert abs(nll[0] + lml[0]) <= ROUTE * abs(lml[0])
    b = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=1)
    b.multi_reserve(1, P)
    b.multi_grad_reserve(1, P)
    bth, blml, bnev = b.optimize_multi_batch(X[None, T - N:T], np.ascontiguousarray(Y[None, T - N:T].transpose(0, 2, 1)), kid, th0, max_evals=200)
    print(f"kid {kid}: evaluations {nev[0]} (batch {bnev[0]}), logml sum {lml[0]} (batch {blml[0]}), theta {th[0]} (batch {bth[0]})")
    assert lml[0] == pytest.approx(blml[0], rel=1e-6, abs=1e-4)
    np.testing.assert_allclose(th[0], bth[0], rtol=2e-3)
    assert abs(int(nev[0]) - int(bnev[0])) <= 3
    assert wmo.jitter(kid, th[0], N, X[:T], Y[:T]) == 0.0
    Xs = wm.points_for(kid, X, T, N, 9, np.random.default_rng(3))
    mean, var, logml = ctx.window_predict_multi(Xs[None])
    om, ov, ol = wm.sliding_window_forecast_multi(kid, th[0], N, X[:T], Y[:T], Xs)
    assert max(wm.errors(mean[0], var[0], logml[0], om, ov, ol)) <= TOL
    out = ctx.window_push_multi(X[None, T:], Y[None, T:])
    pm, pv, lm = ao.stream_ticks(kid, th[0], N, X, Y[:, 0], T, T + K)
    assert np.max(np.abs(out[0][0] - pm)) <= TOL * max(np.max(np.abs(pm)), np.max(np.sqrt(pv)))
    assert np.max(np.abs(out[1][0] - pv) / pv) <= TOL and np.max(np.abs(out[2][0] - lm) / np.maximum(np.abs(lm), 1.0)) <= TOL


def test_optimize_multi_leaves_unselected_windows_alone_and_rejects_a_bad_start(engine):
    kid, N, d, P, T, seed = wmo.OPT_CASES[0]
    W, K = 3, 3
    X, Y = streams(W, T + K, d, P, seed)
    th0 = wmo.opt_start(kid, d)
    a, b = new_ctx(engine, W, N, d, kid, th0, P), new_ctx(engine, W, N, d, kid, th0, P)
    for c in (a, b):
        c.window_push_multi(X[:, :T], Y[:, :T])
    sel = np.array([1, 0, 1], dtype=bool)
    th, lml, nev = a.window_optimize_multi(max_evals=200, select=sel)
    assert np.all(np.isnan(th[1])) and np.isnan(lml[1]) and nev[1] == 0 and np.all(nev[sel] > 1) and np.all(th[sel] > 0)
    na, ga, la = a.window_multi_nll_grad()
    nb, gb, lb = b.window_multi_nll_grad()
    assert na[1] == nb[1] and np.array_equal(ga[1], gb[1]) and np.array_equal(la[1], lb[1])
    assert np.max(np.abs(na[sel] + lml[sel]) / np.abs(lml[sel])) <= ROUTE and np.all(-na[sel] >= -nb[sel] - 1e-9)
    Xs = X[:, T - 5:T] + 0.3
    for u, v in zip(a.window_predict_multi(Xs) + a.window_push_multi(X[:, T:], Y[:, T:]),
                    b.window_predict_multi(Xs) + b.window_push_multi(X[:, T:], Y[:, T:])):
        assert np.array_equal(u[1], v[1])
    # a start theta <= 0 in a selected window: rejected, nothing changes
    neg = np.tile(th0, (W, 1))
    neg[2, -1] = -1e-3
    b.window_set_theta(neg, select=np.array([0, 0, 1], dtype=bool), check=False)
    before = b.window_multi_nll_grad()
    assert b.lib.cgp_window_optimize_multi(b.h, P, 50, None, None, 0, None, None) == EINVAL
    for u, v in zip(before, b.window_multi_nll_grad()):
        assert np.array_equal(u, v, equal_nan=True)
    th2, _, nev2 = b.window_optimize_multi(max_evals=50, select=np.array([1, 1, 0], dtype=bool))   # the others still optimise
    assert np.all(nev2[:2] > 1) and nev2[2] == 0


def test_status_codes(engine):
    buf = np.zeros(64)
    p, a = engine._p(buf), buf.ctypes.data
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    lib, h = ctx.lib, ctx.h

    def all_four(P=2):
        return (lib.cgp_window_multi_nll_grad(h, P, p, p, 4, p), lib.cgp_window_multi_nll_grad_device(h, P, a, a, 4, a, None),
                lib.cgp_window_optimize_multi(h, P, 10, None, None, 0, None, None))

    # no windows
    assert lib.cgp_window_multi_grad_reserve(h) == ESTATE and all_four() == (ESTATE,) * 3
    theta = wm.theta_of(2, 1)
    ctx.window_init(1, 8, 1, 2, theta)
    # before cgp_window_multi_reserve
    assert lib.cgp_window_multi_grad_reserve(h) == ESTATE and all_four() == (ESTATE,) * 3
    ctx.window_multi_reserve(2)
    # the objective's own reservation missing
    assert all_four() == (ESTATE,) * 3
    assert lib.cgp_window_multi_grad_reserve(h) == 0 and lib.cgp_window_multi_grad_reserve(h) == 0   # replaced
    # cgp_window_multi_reserve (windows still empty) drops the objective's scratch with the reservation it was sized for
    assert lib.cgp_window_multi_reserve(h, 2) == 0 and all_four() == (ESTATE,) * 3 and lib.cgp_window_multi_grad_reserve(h) == 0
    # P is not the reservation's, NULL nll / grad, grad_stride < ntheta
    assert all_four(3) == (EINVAL,) * 3
    assert lib.cgp_window_multi_nll_grad(h, 2, None, p, 4, p) == EINVAL and lib.cgp_window_multi_nll_grad(h, 2, p, None, 4, p) == EINVAL
    assert lib.cgp_window_multi_nll_grad_device(h, 2, None, a, 4, a, None) == EINVAL
    assert lib.cgp_window_multi_nll_grad_device(h, 2, a, None, 4, a, None) == EINVAL
    assert lib.cgp_window_multi_nll_grad(h, 2, p, p, 3, p) == EINVAL and lib.cgp_window_multi_nll_grad_device(h, 2, a, a, 3, a, None) == EINVAL
    assert lib.cgp_window_optimize_multi(h, 2, 10, None, p, 3, None, None) == EINVAL
    # any fill state: after pushes the reservation can be made again, and the context works
    X, Y = wm.stream(12, 1, 2, 3)
    ctx.window_push_multi(X[None], Y[None])
    assert lib.cgp_window_multi_grad_reserve(h) == 0
    nll, g, logml = ctx.window_multi_nll_grad()
    close(nll[0], g[0], logml[0], 2, theta, 8, X, Y)
    # cgp_window_init drops both reservations
    ctx.window_init(1, 8, 1, 2, theta)
    assert all_four() == (ESTATE,) * 3
    ctx.window_multi_reserve(2)
    assert all_four() == (ESTATE,) * 3
    # an fp32 context: CGP_EINVAL before anything is enqueued, with or without windows
    c32 = engine.Context(max_n=8, max_m=8, max_d=1, dtype=engine.F32)
    l32, h32 = c32.lib, c32.h
    for _ in range(2):
        assert l32.cgp_window_multi_grad_reserve(h32) == EINVAL
        assert l32.cgp_window_multi_nll_grad(h32, 2, p, p, 4, p) == EINVAL
        assert l32.cgp_window_multi_nll_grad_device(h32, 2, a, a, 4, a, None) == EINVAL
        assert l32.cgp_window_optimize_multi(h32, 2, 10, None, None, 0, None, None) == EINVAL
        c32.window_init(1, 8, 1, 2, theta)
