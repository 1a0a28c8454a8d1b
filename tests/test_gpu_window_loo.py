"""GPU tests of leave-one-out cross-validation of the resident sliding windows (cgp_window_loo, cgp_window_loo_device) against
tests/loo_oracle.py on the window's samples in their own order (oldest first), through the C ABI.  Bar: the project's fp64 bar,
1e-6, in loo_oracle.check's metric (see tests/test_gpu_loo.py)."""
import numpy as np
import pytest

from adapt_oracle import window_of
import loo_oracle as lo
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
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)]), y


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def check_window(out, w, kid, theta, N, X, y, t, tol=TOL):
    """Window w after t ticks of (X, y): entries [0, n) against the oracle on the window's samples in order, [n, N) NaN."""
    mean, var, lpd, tot = (o[w] for o in out)
    Xw, yw = window_of(N, X, y, t)
    n = len(yw)
    want = lo.loo(kid, theta, Xw, yw)
    e = lo.check((mean[:n], var[:n], lpd[:n], tot), want, yw, tol)
    print(f"window {w}, t = {t}: errors / bar: mean {e[0] / tol:.3g} var {e[1] / tol:.3g} lpd {e[2] / tol:.3g} sum {e[3] / tol:.3g}")
    assert all(np.all(np.isnan(a[n:])) for a in (mean, var, lpd))
    return want


def test_a_stream_through_a_window_at_every_chunk_edge(engine):
    """N = 48: while filling at n = 1, 15, 16, 17, 33, when full, and after 2 N + 5 ticks (the window has slid and its origin has
    been moved back); agreement with cgp_loo_batch on a host copy of the same samples at the same bar."""
    N, d, kid = 48, 2, 1
    T = 2 * N + 5
    X, y = stream(T, d, 40)
    theta = theta_of(kid, d)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta)
    batch = engine.Context(max_n=N, max_m=N, max_d=d)
    fed = 0
    for t in (1, 15, 16, 17, 33, 48, T):
        ctx.window_push(X[fed:t][None], y[fed:t][None])
        fed = t
        out = ctx.window_loo()
        assert out[0].shape == (1, N) and ctx.window_state(0) == (min(t, N), 0)
        check_window(out, 0, kid, theta, N, X, y, t)
        Xw, yw = window_of(N, X, y, t)
        n = len(yw)
        rc, bm, bv, bl, bs, _, _ = batch.loo_batch(Xw[None], yw[None], theta[None], kid)
        assert rc == 0
        lo.check((out[0][0, :n], out[1][0, :n], out[2][0, :n], out[3][0]), lo.Loo(bm[0], bv[0], bl[0], bs[0], None, 0.0), yw)


def test_the_configs3_window(engine):
    """N = 512, d = 3 after 700 ticks: 32 chunks, the longest substitution 31 blocks."""
    N, d, T = 512, 3, 700
    X, y = stream(T, d, 7)
    theta = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    ctx.window_push(X[None], y[None])
    check_window(ctx.window_loo(), 0, 1, theta, N, X, y, T)


@pytest.mark.parametrize("kid,d", [(0, 2), (1, 3), (2, 1), (3, 2), (4, 6)])
def test_every_kernel_five_windows(engine, kid, d):
    """5 windows of N = 40 (3 chunks each: windows x chunks is no multiple of the 4 waves of a workgroup), each with its own
    stream and theta, two of them checked after the window has slid, all while it fills."""
    W, N = 5, 40
    T = N + 13
    Xw, yw = zip(*[stream(T, d, 100 * kid + w, tick0=11 + 3 * w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(kid, d), (W, 1))
    theta[:, 0] *= 1.0 + 0.1 * np.arange(W)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    ctx.window_push(X[:, :21], y[:, :21])
    out = ctx.window_loo()
    for w in range(W):
        check_window(out, w, kid, theta[w], N, X[w], y[w], 21)
    ctx.window_push(X[:, 21:], y[:, 21:])
    out = ctx.window_loo()
    for w in range(W):
        check_window(out, w, kid, theta[w], N, X[w], y[w], T)


def test_empty_and_failed_windows(engine):
    """Before any push: NaN rows and lpd_sum = 0.  Window 1 of three fails at its first tick (sigma_n^2 < -sigma_f^2): NaN
    everywhere, lpd_sum included; the other two are right, and bitwise what they are in a context without the failed window's
    theta (same slots)."""
    W, N, d, T = 3, 24, 1, 70
    Xw, yw = zip(*[stream(T, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    bad = theta.copy()
    bad[1, -1] = -2.0 * bad[1, 0]
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    a.window_init(W, N, d, 0, bad)
    b.window_init(W, N, d, 0, theta)
    mean, var, lpd, tot = a.window_loo()
    assert all(np.all(np.isnan(o)) for o in (mean, var, lpd)) and np.array_equal(tot, np.zeros(W))
    with pytest.raises(engine.CgpError):
        a.window_push(X, y)
    b.window_push(X, y)
    assert a.window_state(1)[1] > 0
    oa, ob = a.window_loo(), b.window_loo()
    assert all(np.all(np.isnan(o[1])) for o in oa)
    for w in (0, 2):
        check_window(oa, w, 0, theta[w], N, X[w], y[w], T)
        assert all(np.array_equal(u[w], v[w]) for u, v in zip(oa, ob))


def test_loo_is_read_only_host_form_is_device_form_and_graph_replay(engine):
    """push A, LOO, then forecast / gradient / push B = the same on a second context that never ran LOO, bitwise; the device form
    on the caller's stream and a captured side stream write the host form's bits; each output alone has the bits it has beside
    the others."""
    import torch
    W, N, d, T, K = 3, 48, 2, 170, 30
    Xw, yw = zip(*[stream(T + K, d, 60 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(1, d), (W, 1)) * (1.0 + 0.1 * np.arange(W))[:, None]
    a, b = engine.Context(max_n=8, max_m=8, max_d=d), engine.Context(max_n=8, max_m=8, max_d=d)
    for c in (a, b):
        c.window_init(W, N, d, 1, theta)
        c.window_push(X[:, :T - 20], y[:, :T - 20])
    a.window_loo()   # once in the middle of the stream as well
    for c in (a, b):
        c.window_push(X[:, T - 20:T], y[:, T - 20:T])
    host = a.window_loo()
    for w in range(W):
        check_window(host, w, 1, theta[w], N, X[w], y[w], T)
    f = lambda *s: torch.full(s, -1.0, dtype=torch.float64, device="cuda")
    outs = [f(W, N), f(W, N), f(W, N), f(W)]
    ptrs = [t.data_ptr() for t in outs]

    def clear():
        for t in outs:
            t.fill_(-1.0)
        torch.cuda.synchronize()

    def check(which=range(4)):
        a.synchronize()
        torch.cuda.synchronize()
        for k, (t, h) in enumerate(zip(outs, host)):
            assert np.array_equal(t.cpu().numpy(), h if k in which else np.full(h.shape, -1.0))

    for s in (0, engine.STREAM_CTX):
        clear()
        assert a.window_loo_device(*ptrs, stream=s) == 0
        check()
    for k in range(4):
        clear()
        assert a.window_loo_device(*[p if i == k else 0 for i, p in enumerate(ptrs)], stream=0) == 0
        check([k])
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert a.window_loo_device(*ptrs, stream=torch.cuda.current_stream().cuda_stream) == 0
    for _ in range(2):
        clear()
        graph.replay()
        check()
    Xs = X[:, T - 9:T] + 0.2
    (ma, va), (mb, vb) = a.window_predict(Xs), b.window_predict(Xs)
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    for u, v in zip(a.window_nll_grad(), b.window_nll_grad()):
        assert np.array_equal(u, v)
    for u, v in zip(a.window_push(X[:, T:], y[:, T:]), b.window_push(X[:, T:], y[:, T:])):
        assert np.array_equal(u, v)
    for u, v in zip(a.window_loo(), b.window_loo()):
        assert np.array_equal(u, v)


def test_fp32_contexts_answer_in_fp64(engine):
    """The window calls are fp64 whatever the context's dtype, as cgp_window_predict is."""
    N, d, T = 40, 2, 60
    X, y = stream(T, d, 3)
    theta = theta_of(1, d)
    outs = []
    for dtype in (0, 1):
        ctx = engine.Context(max_n=8, max_m=8, max_d=d, dtype=dtype)
        ctx.window_init(1, N, d, 1, theta)
        ctx.window_push(X[None], y[None])
        outs.append(ctx.window_loo())
    for u, v in zip(*outs):
        assert np.array_equal(u, v)


def test_error_paths(engine):
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    buf = np.zeros(64)
    p = engine._p(buf)
    lib = ctx.lib
    assert lib.cgp_window_loo(None, p, p, p, p) == ESTATE and lib.cgp_window_loo_device(None, None, None, None, None, None) == ESTATE
    assert lib.cgp_window_loo(ctx.h, p, p, p, p) == ESTATE   # no windows yet
    assert lib.cgp_window_loo_device(ctx.h, buf.ctypes.data, None, None, None, None) == ESTATE
    ctx.window_init(1, 8, 1, 2, theta_of(2, 1))
    assert lib.cgp_window_loo(ctx.h, None, None, None, None) == EINVAL
    assert lib.cgp_window_loo_device(ctx.h, None, None, None, None, None) == EINVAL
    X, y = stream(5, 1, 1)
    ctx.window_push(X[None], y[None])
    mean, var, lpd, tot = ctx.window_loo()
    assert np.all(np.isfinite(mean[0, :5])) and np.all(np.isnan(mean[0, 5:])) and np.isfinite(tot[0])
