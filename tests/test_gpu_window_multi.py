"""GPU tests of the multi-target sliding windows (cgp_window_multi_reserve, cgp_window_push_multi[_device],
cgp_window_predict_multi[_device]): P target columns share a window's resident factor.  Parity against the per-column refit
oracle tests/window_multi_oracle.py at the project's fp64 bar, 1e-6, in the metric of the multi-target fits (the mean per column
against that column's largest oracle mean, var relative, logml against max(1, |logml|)); routes bitwise.  The largest errors and
the gap between column 0's mean row and cgp_window_predict's are printed; DESIGN.md section 9h records them."""
import numpy as np
import pytest

import forecast_oracle as fo
import window_multi_oracle as wm
import test_gpu_window_paths as paths

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h
WORST = {"mean": 0.0, "var": 0.0, "logml": 0.0, "col0": 0.0}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def new_ctx(engine, W, N, d, kid, theta, P):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    if P:
        ctx.window_multi_reserve(P)
    return ctx


def streams(W, T, d, P, seed):
    Xw, Yw = zip(*[wm.stream(T, d, P, seed + 17 * w) for w in range(W)])
    return np.stack(Xw), np.stack(Yw)


def close(mean, var, logml, kid, theta, N, X, Y, Xs, noise=True, what=""):
    """One window: mean (P, M), var (M,), logml (P,) against the refit of the stream's last N samples."""
    om, ov, ol, jit = wm.sliding_window_forecast_multi(kid, theta, N, X, Y, Xs, noise, want_jitter=True)
    assert jit == 0.0, what   # the oracle's window is positive definite as it stands
    em, ev, el = wm.errors(mean, var, logml, om, ov, ol)
    for k, e in (("mean", em), ("var", ev), ("logml", el)):
        WORST[k] = max(WORST[k], e)
    print(f"{what} errors / bar: mean {em / TOL:.3g} var {ev / TOL:.3g} logml {el / TOL:.3g}")
    assert em <= TOL and ev <= TOL and el <= TOL, (what, em, ev, el)


PARITY = [(2, 16, 1), (2, 17, 1), (0, 33, 2), (1, 64, 3), (1, 48, 8), (3, 40, 2), (4, 64, 3)]


@pytest.mark.parametrize("P", [1, 3, 16, 17])
@pytest.mark.parametrize("kid,N,d", PARITY)
def test_forecast_matches_the_refit_oracle_over_the_rings_states(engine, kid, N, d, P):
    """Three windows fed uneven pushes (1, 2, 5, 37, 3, 11, ... ticks, cut again at N, 2N - 1, 2N, 2N + 1 so that the first full
    tick and both sides of the ring's compaction are forecast from) up to 2N + 8 ticks: after every push M = 40, 17 and 1 test
    points, var bitwise cgp_window_predict's, column 0's mean beside cgp_window_predict's."""
    W, T = 3, 2 * N + 8
    X, Y = streams(W, T, d, P, 1000 * kid + N)
    theta = wm.theta_of(kid, d)
    rng = np.random.default_rng(N + P)
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    cuts, t = {N, 2 * N - 1, 2 * N, 2 * N + 1, 2 * N + 3, T}, 0
    for s in [1, 2, 5, 37, 3, 11] * 40:
        t += s
        cuts.add(min(t, T))
    fed = 0
    for t in sorted(cuts):
        ctx.window_push_multi(X[:, fed:t], Y[:, fed:t])
        fed = t
        assert ctx.window_state(W - 1) == (min(N, t), 0)
        Xs = np.stack([wm.points_for(kid, X[w], t, N, 40, rng) for w in range(W)])
        noise = bool(t & 1)
        for M in (40, 17, 1):
            mean, var, logml = ctx.window_predict_multi(Xs[:, :M], include_noise=noise)
            assert mean.shape == (W, P, M) and var.shape == (W, M) and logml.shape == (W, P)
            m0, v0 = ctx.window_predict(Xs[:, :M], include_noise=noise)
            assert np.array_equal(var, v0)
            for w in range(W):
                if M == 40 or w == 0:
                    close(mean[w], var[w], logml[w], kid, theta, N, X[w, :t], Y[w, :t], Xs[w, :M], noise, what=f"t {t} M {M} w {w}")
                om0, _ = (fo.sliding_window_forecast(kid, theta, N, X[w, :t], Y[w, :t, 0], Xs[w, :M], noise) if kid < 3
                          else wm.sliding_window_forecast_multi(kid, theta, N, X[w, :t], Y[w, :t, :1], Xs[w, :M], noise)[:2])
                scale = np.max(np.abs(om0))
                assert np.max(np.abs(m0[w] - np.reshape(om0, -1))) <= TOL * scale   # cgp_window_predict's own mean, same bar
                WORST["col0"] = max(WORST["col0"], np.max(np.abs(mean[w, 0] - m0[w])) / scale)
    print("largest errors so far:", WORST)


@pytest.mark.parametrize("N,d,T", [(700, 3, 1500), (1536, 2, 1700)])
def test_the_two_longer_forms(engine, N, d, T):
    """512 < N <= 1024 (sixteen test points / target columns per workgroup) and N > 1024 (eight): P = 3, M = 9."""
    P, M = 3, 9
    X, Y = wm.stream(T, d, P, N)
    theta = wm.theta_of(1, d)
    ctx = new_ctx(engine, 1, N, d, 1, theta, P)
    ctx.window_push_multi(X[None], Y[None])
    Xs = wm.points_for(1, X, T, N, M, np.random.default_rng(4))
    mean, var, logml = ctx.window_predict_multi(Xs[None])
    _, v0 = ctx.window_predict(Xs[None])
    assert np.array_equal(var, v0)
    close(mean[0], var[0], logml[0], 1, theta, N, X, Y, Xs, what=f"N {N}")


@pytest.mark.parametrize("W,N,d,kid", [(5, 48, 2, 1), (512, 64, 1, 2)])
def test_push_outputs_are_bitwise_the_single_target_push_of_column_0(engine, W, N, d, kid):
    """A twin context without a reservation fed column 0 through cgp_window_push: every tick's outputs equal bitwise, over the
    filling, the steady state (two ticks per pass; four from 512 windows) and the compaction; so do the forecasts' var."""
    P, T = 4, 2 * N + 13
    X, Y = streams(W, T, d, P, 3 + W)
    theta = wm.theta_of(kid, d)
    multi, twin = new_ctx(engine, W, N, d, kid, theta, P), new_ctx(engine, W, N, d, kid, theta, 0)
    fed = 0
    for t in (1, 3, N - 1, N + 22, 2 * N - 2, T):
        a = multi.window_push_multi(X[:, fed:t], Y[:, fed:t])
        b = twin.window_push(X[:, fed:t], Y[:, fed:t, 0])
        fed = t
        for u, v in zip(a, b):
            assert np.array_equal(u, v), t
    Xs = X[:, -7:] + 0.25
    mean, var, logml = multi.window_predict_multi(Xs)
    m0, v0 = twin.window_predict(Xs)
    assert np.array_equal(var, v0)
    for w in (0, W - 1):
        close(mean[w], var[w], logml[w], kid, theta, N, X[w], Y[w], Xs[w], what=f"W {W} w {w}")


def test_a_column_does_not_depend_on_its_place_its_company_its_slot_or_its_neighbours(engine):
    """Permuting the columns permutes the outputs; the first 3 of 17 columns equal those 3 run alone; a window in slot 0 of 1
    equals the same window in slot 4 of 5.  Bitwise.  (Every context is fed tick by tick: the same push kernel everywhere.)"""
    N, d, kid, T, M, P = 40, 2, 1, 57, 21, 17
    X, Y = streams(5, T, d, P, 77)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -M:] + 0.2
    perm = np.random.default_rng(5).permutation(P)

    def run(Xc, Yc, Xq):
        ctx = new_ctx(engine, len(Xc), N, d, kid, theta, Yc.shape[2])
        for i in range(T):
            ctx.window_push_multi(Xc[:, i:i + 1], Yc[:, i:i + 1])
        return ctx.window_predict_multi(Xq)

    mean, var, logml = run(X, Y, Xs)
    pmean, pvar, plogml = run(X, Y[:, :, perm], Xs)
    assert np.array_equal(pmean, mean[:, perm]) and np.array_equal(plogml, logml[:, perm]) and np.array_equal(pvar, var)
    m3, v3, l3 = run(X, Y[:, :, :3], Xs)
    assert np.array_equal(m3, mean[:, :3]) and np.array_equal(l3, logml[:, :3]) and np.array_equal(v3, var)
    m1, v1, l1 = run(X[4:], Y[4:], Xs[4:])
    assert np.array_equal(m1[0], mean[4]) and np.array_equal(l1[0], logml[4]) and np.array_equal(v1[0], var[4])


def test_host_device_and_graph_replay_agree_bitwise(engine):
    """Also: logml = NULL leaves mean / var identical, and two forecasts in a row are identical."""
    import torch
    W, N, d, kid, T, M, P = 3, 40, 3, 1, 100, 53, 5
    X, Y = streams(W, T, d, P, 500)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -M:] + 0.2
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    ctx.window_push_multi(X, Y)
    ref = ctx.window_predict_multi(Xs)
    again = ctx.window_predict_multi(Xs)
    for a, b in zip(ref, again):
        assert np.array_equal(a, b)
    mean, var, none = ctx.window_predict_multi(Xs, want_logml=False)
    assert none is None and np.array_equal(mean, ref[0]) and np.array_equal(var, ref[1])
    dxs = torch.from_numpy(Xs).cuda()
    out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((W, P, M), (W, M), (W, P))]

    def clear():
        for t in out:
            t.fill_(-1.0)
        torch.cuda.synchronize()

    def check(n=3):
        ctx.synchronize()
        torch.cuda.synchronize()
        for t, r in list(zip(out, ref))[:n]:
            assert np.array_equal(t.cpu().numpy(), r)

    def enqueue(s, logml=True):
        ptrs = [t.data_ptr() for t in out]
        assert ctx.window_predict_multi_device(M, P, dxs.data_ptr(), True, ptrs[0], ptrs[1], ptrs[2] if logml else 0, stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    clear()
    enqueue(0, logml=False)
    check(2)
    assert np.all(out[2].cpu().numpy() == -1.0)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()


def test_push_multi_device_equals_the_host_push(engine):
    import torch
    W, N, d, kid, P = 3, 24, 2, 1, 3
    T1, T2 = 31, 300   # the second push is longer than the block column 0 is gathered into: it grows
    X, Y = streams(W, T1 + T2, d, P, 9)
    theta = wm.theta_of(kid, d)
    host, dev = new_ctx(engine, W, N, d, kid, theta, P), new_ctx(engine, W, N, d, kid, theta, P)
    Xs = X[:, -6:] + 0.3
    for lo, hi in ((0, T1), (T1, T1 + T2)):
        T = hi - lo
        ref = host.window_push_multi(X[:, lo:hi], Y[:, lo:hi])
        dx, dY = torch.from_numpy(X[:, lo:hi].copy()).cuda(), torch.from_numpy(Y[:, lo:hi].copy()).cuda()
        out = [torch.full((W, T), -1.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        assert dev.window_push_multi_device(T, P, dx.data_ptr(), dY.data_ptr(), True, *[t.data_ptr() for t in out]) == 0
        dev.synchronize()
        torch.cuda.synchronize()
        for t, r in zip(out, ref):
            assert np.array_equal(t.cpu().numpy(), r)
        for a, b in zip(host.window_predict_multi(Xs), dev.window_predict_multi(Xs)):
            assert np.array_equal(a, b)


def test_forecast_does_not_touch_the_windows(engine):
    """push A, forecasts, push B = push A, push B on a second context, bitwise: the outputs of B, the state words, and every
    window call after it (forecast, leave-one-out -- which reads the samples --, the multi-target forecast)."""
    W, N, d, kid, P, T = 2, 48, 2, 1, 3, 170
    X, Y = streams(W, T, d, P, 70)
    theta = wm.theta_of(kid, d)
    Xs = X[:, -30:] + 0.1
    outs = []
    for between in (True, False):
        ctx = new_ctx(engine, W, N, d, kid, theta, P)
        ctx.window_push_multi(X[:, :90], Y[:, :90])
        if between:
            ctx.window_predict_multi(Xs)
            ctx.window_predict_multi(Xs[:, :3], include_noise=False, want_logml=False)
        o = ctx.window_push_multi(X[:, 90:], Y[:, 90:]) + ctx.window_predict(Xs) + ctx.window_loo() + ctx.window_predict_multi(Xs)
        outs.append(o + (np.array([ctx.window_state(w) for w in range(W)]),))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_set_theta_needs_no_further_call(engine):
    """After cgp_window_set_theta the next multi-target forecast meets the oracle at the new theta for all columns."""
    W, N, d, kid, P, T, M = 3, 40, 3, 1, 5, 95, 19
    X, Y = streams(W, T, d, P, 21)
    theta = wm.theta_of(kid, d)
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    ctx.window_push_multi(X, Y)
    new = np.stack([theta * (1.0 + 0.15 * (w + 1)) for w in range(W)])
    ctx.window_set_theta(new)
    Xs = X[:, -M:] + 0.2
    mean, var, logml = ctx.window_predict_multi(Xs)
    for w in range(W):
        close(mean[w], var[w], logml[w], kid, new[w], N, X[w], Y[w], Xs[w], what=f"new theta, window {w}")


def test_failed_window_answers_nan_and_is_revived_for_every_column(engine):
    """The failure recipe of tests/test_gpu_window_paths.py (a repeated input under a negative noise variance) in mid-stream:
    the victim answers NaN in all P mean rows, var and logml, the neighbours are bitwise what they are beside a healthy one; after a
    reviving set_theta it meets the oracle for every column, the samples pushed while it was failed included."""
    kid, W, N, d, P, victim, pre, T, tl, K, M = 1, 3, 32, 2, 3, 1, 41, 9, 4, 6, 11
    ts = pre + tl
    X, y, bad, good = paths.failing_streams(kid, W, d, pre + T + K, 31, victim, ts)
    paths.assert_numpy_fails_at(kid, bad[victim], N, X[victim], ts)
    rng = np.random.default_rng(8)
    Y = np.stack([y] + [y * (1.5 + p) + rng.normal(0, 0.02, y.shape) for p in range(1, P)], axis=2)
    others = np.arange(W) != victim
    A, B = new_ctx(engine, W, N, d, kid, bad, P), new_ctx(engine, W, N, d, kid, good, P)
    for c in (A, B):
        c.window_push_multi(X[:, :pre], Y[:, :pre])
    *oa, rc = A.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T], check=False)
    ob = B.window_push_multi(X[:, pre:pre + T], Y[:, pre:pre + T])
    assert rc == tl + 1 and A.window_state(victim) == (N, tl + 1)
    for u, v in zip(oa, ob):
        assert np.array_equal(u[others], v[others])
    Xs = X[:, pre + T - M:pre + T] + 0.25
    mean, var, logml, code = A.window_predict_multi(Xs, check=False)
    mb, vb, lb = B.window_predict_multi(Xs)
    assert code == tl + 1
    with pytest.raises(engine.CgpError):
        A.window_predict_multi(Xs)
    assert np.all(np.isnan(mean[victim])) and np.all(np.isnan(var[victim])) and np.all(np.isnan(logml[victim]))
    for a, b in ((mean, mb), (var, vb), (logml, lb)):
        assert np.array_equal(a[others], b[others]) and not np.any(np.isnan(a[others]))
    # more samples while it is failed, then the revival
    *_, rc = A.window_push_multi(X[:, pre + T:], Y[:, pre + T:], check=False)
    assert rc == tl + 1
    _, info = A.window_set_theta(good, select=~others)
    assert np.all(info == 0) and A.window_state(victim) == (N, 0)
    Xs = X[:, -M:] + 0.25
    mean, var, logml = A.window_predict_multi(Xs)
    for w in range(W):
        close(mean[w], var[w], logml[w], kid, good[w], N, X[w], Y[w], Xs[w], what=f"revived, window {w}")


def test_empty_windows_answer_with_the_prior(engine):
    W, N, d, kid, P, M = 2, 16, 1, 2, 3, 5
    theta = wm.theta_of(kid, d)
    ctx = new_ctx(engine, W, N, d, kid, theta, P)
    Xs = np.array([-4.0, 0.0, 7.0, 2.5, 30.0])[None, :, None].repeat(W, axis=0)
    for noise in (True, False):
        mean, var, logml = ctx.window_predict_multi(Xs, include_noise=noise)
        om, ov, ol = wm.prior(kid, theta, Xs[0], P, noise)
        assert np.all(mean == 0.0) and np.all(logml == 0.0)
        np.testing.assert_allclose(var[0], ov, rtol=1e-14)
        assert np.array_equal(var[0], var[1])


def test_status_codes(engine):
    buf = np.zeros(64)
    p, a = engine._p(buf), buf.ctypes.data
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    lib, h = ctx.lib, ctx.h
    # no windows
    assert lib.cgp_window_multi_reserve(h, 2) == ESTATE
    assert lib.cgp_window_push_multi(h, 1, 2, p, p, 1, p, p, p) == ESTATE
    assert lib.cgp_window_push_multi_device(h, 1, 2, a, a, 1, a, a, a, None) == ESTATE
    assert lib.cgp_window_predict_multi(h, 1, 2, p, 1, p, p, p) == ESTATE
    assert lib.cgp_window_predict_multi_device(h, 1, 2, a, 1, a, a, a, None) == ESTATE
    theta = wm.theta_of(2, 1)
    ctx.window_init(1, 8, 1, 2, theta)
    # no reservation
    assert lib.cgp_window_push_multi(h, 1, 2, p, p, 1, p, p, p) == ESTATE
    assert lib.cgp_window_predict_multi(h, 1, 2, p, 1, p, p, p) == ESTATE
    assert lib.cgp_window_predict_multi_device(h, 1, 2, a, 1, a, a, a, None) == ESTATE
    # P = 0 or 65
    assert lib.cgp_window_multi_reserve(h, 0) == EINVAL and lib.cgp_window_multi_reserve(h, 65) == EINVAL
    assert lib.cgp_window_multi_reserve(h, 64) == 0 and lib.cgp_window_multi_reserve(h, 2) == 0   # replaced while still empty
    ctx._win_p = 2
    # P mismatch, M < 1, T < 1, NULL pointers
    assert lib.cgp_window_push_multi(h, 1, 3, p, p, 1, p, p, p) == EINVAL
    assert lib.cgp_window_predict_multi(h, 1, 3, p, 1, p, p, p) == EINVAL
    assert lib.cgp_window_predict_multi_device(h, 1, 1, a, 1, a, a, a, None) == EINVAL
    assert lib.cgp_window_predict_multi(h, 0, 2, p, 1, p, p, p) == EINVAL
    assert lib.cgp_window_predict_multi_device(h, 0, 2, a, 1, a, a, a, None) == EINVAL
    assert lib.cgp_window_push_multi(h, 0, 2, p, p, 1, p, p, p) == EINVAL
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert lib.cgp_window_predict_multi(h, 1, 2, args[0], 1, args[1], args[2], p) == EINVAL
    for k in range(5):
        args = [a, a, a, a, a]
        args[k] = None
        assert lib.cgp_window_push_multi_device(h, 1, 2, args[0], args[1], 1, args[2], args[3], args[4], None) == EINVAL
    # a plain push on a reserved context
    assert lib.cgp_window_push(h, 1, p, p, 1, p, p, p) == ESTATE
    assert lib.cgp_window_push_device(h, 1, a, a, 1, a, a, a, None) == ESTATE
    # the context stays usable; a reservation on windows that are no longer empty
    X, Y = wm.stream(12, 1, 2, 3)
    ctx.window_push_multi(X[None], Y[None])
    assert lib.cgp_window_multi_reserve(h, 2) == ESTATE
    Xs = X[-1:] + 1.0 + np.arange(5.0)[:, None]
    mean, var, logml = ctx.window_predict_multi(Xs[None])
    close(mean[0], var[0], logml[0], 2, theta, 8, X, Y, Xs)
    # the reservation goes with a re-initialisation, and plain pushes are back
    ctx.window_init(1, 8, 1, 2, theta)
    assert lib.cgp_window_predict_multi(h, 1, 2, p, 1, p, p, p) == ESTATE
    ctx.window_push(X[None], Y[None, :, 0])
    assert lib.cgp_window_multi_reserve(h, 2) == ESTATE   # not empty
    # an fp32 context: CGP_EINVAL before anything is enqueued, with or without windows
    c32 = engine.Context(max_n=8, max_m=8, max_d=1, dtype=engine.F32)
    assert c32.lib.cgp_window_multi_reserve(c32.h, 2) == EINVAL
    c32.window_init(1, 8, 1, 2, theta)
    assert c32.lib.cgp_window_multi_reserve(c32.h, 2) == EINVAL
    assert c32.lib.cgp_window_push_multi(c32.h, 1, 2, p, p, 1, p, p, p) == EINVAL
    assert c32.lib.cgp_window_predict_multi(c32.h, 1, 2, p, 1, p, p, p) == EINVAL
    assert c32.lib.cgp_window_predict_multi_device(c32.h, 1, 2, a, 1, a, a, a, None) == EINVAL
    c32.window_push(X[None], Y[None, :, 0])
