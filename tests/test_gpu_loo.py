"""GPU parity of leave-one-out cross-validation after batch / single fits (cgp_loo, cgp_loo_batch, cgp_loo_batch_device) against
tests/loo_oracle.py, through the C ABI.  Bar: the project's fp64 bar, 1e-6, in loo_oracle.check's metric
    |d loo_mean| <= 1e-6 max(1, max|y|)      |d loo_var| <= 1e-6 loo_var
    |d loo_lpd_i| <= 1e-6 max(1, |loo_lpd_i|)      |d lpd_sum| <= 1e-6 max(1, sum|loo_lpd_i|)
(the oracle's closed form and N brute-force refits agree to <= 7e-13 in loo_lpd on these windows: tests/test_oracle_loo.py)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
import loo_oracle as lo
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


def window(N, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [rng.normal(size=N) for _ in range(d - 1)]), y


def problem(B, N, d, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, yw = zip(*[window(N, d, seed + 17 * b, tick0=11 + b) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return np.stack(Xw), np.stack(yw), theta


def ctx_for(engine, B, N, d):
    return engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)


def check_fit(out, b, kid, theta, X, y, tol=TOL):
    """Fit b of a loo_batch result against the oracle (logML at 1e-9 relative); returns the oracle's record."""
    rc, mean, var, lpd, tot, logml, info = out
    want = lo.loo(kid, theta, X, y)
    e = lo.check((mean[b], var[b], lpd[b], tot[b]), want, y, tol)
    print(f"fit {b}: errors / bar: mean {e[0] / tol:.3g} var {e[1] / tol:.3g} lpd {e[2] / tol:.3g} sum {e[3] / tol:.3g}")
    assert info[b] == 0 and abs(logml[b] - want.logml) <= 1e-9 * abs(want.logml)
    return want


def same(a, b, rows=slice(None)):
    """Bitwise equality of the per-sample outputs and sums of two loo_batch results (NaN equal to NaN)."""
    return all(np.array_equal(u[rows], v[rows], equal_nan=True) for u, v in zip(a[1:6], b[1:6]))


GOLDEN = ["sk_se_iso_n256_d3", "sk_se_ard_n134_d6", "sk_se_ard_n15_d3", "sk_se_ard_n2_d1", "mp_rbfbrownian_n134",
          "sk_se_ard_n256_d6", "matern_sk_m32_n256_d3", "matern_sk_m52_n256_d3", "matern_mp_m32_n134", "matern_mp_m52_n134"]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_windows_every_kernel(engine, name):
    g = load_golden(name)
    X, y, theta, kid = g["X"], g["y"], g["theta"], int(g["kernel_id"])
    X = X[:, None] if X.ndim == 1 else X
    N, d = X.shape
    ctx = ctx_for(engine, 1, N, d)
    out = ctx.loo_batch(X[None], y[None], theta[None], kid)
    assert out[0] == 0
    check_fit(out, 0, kid, theta, X, y)
    assert abs(out[5][0] - float(g["logml"])) <= 1e-9 * abs(float(g["logml"]))


@pytest.mark.parametrize("src,pin", [("mp_rbfbrownian_n134", "loo_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_mp_m32_n134"),
                                     ("matern_mp_m52_n134", "loo_mp_m52_n134")])
def test_mpmath_pins(engine, src, pin):
    """The 50-digit values themselves, not the float64 oracle."""
    g, p = load_golden(src), load_golden(pin)
    X, y, theta, kid = g["X"], g["y"], g["theta"], int(g["kernel_id"])
    ctx = ctx_for(engine, 1, len(y), 1)
    mean, var, lpd, tot = ctx.loo(X, y, kid, theta)
    lo.check((mean, var, lpd, tot), lo.Loo(p["loo_mean"], p["loo_var"], p["loo_lpd"], float(p["lpd_sum"]), None, 0.0), y)


@pytest.mark.parametrize("d", [1, 3, 6])
@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257])
def test_tile_edges(engine, N, d):
    """One tile, the tile edge, and three block steps with a one-row last tile; two fits, kernels alternating with the shape."""
    kid = (1, 3, 4, 0)[(N + d) % 4] if d > 1 else (2, 0, 3)[N % 3]
    X, y, theta = problem(2, N, d, kid, 100 * N + d)
    ctx = ctx_for(engine, 2, N, d)
    out = ctx.loo_batch(X, y, theta, kid)
    assert out[0] == 0 and out[1].shape == (2, N)
    for b in range(2):
        check_fit(out, b, kid, theta[b], X[b], y[b])


def test_n1_and_n2_closed_forms(engine):
    """N = 1: loo_mean = 0 and loo_var = k(x, x) + sigma_n^2 + 1e-8 (the prior); N = 2: the 2 x 2 inverse written out."""
    th = np.array([0.8, 0.9, 0.02])
    ctx = ctx_for(engine, 1, 2, 1)
    mean, var, lpd, tot = ctx.loo(np.array([[0.3]]), np.array([0.7]), 0, th)
    c = th[0] + th[2] + 1e-8
    assert abs(mean[0]) <= 1e-15 and abs(var[0] - c) <= 1e-12 * c
    assert abs(lpd[0] - (-0.5 * np.log(2 * np.pi * c) - 0.5 * 0.49 / c)) <= 1e-12 and tot == lpd[0]
    xa, xb, ya, yb = 0.1, 0.9, 0.5, -0.2
    b = th[0] * np.exp(-0.5 * (xa - xb) ** 2 / th[1] ** 2)
    mean, var, lpd, tot = ctx.loo(np.array([[xa], [xb]]), np.array([ya, yb]), 0, th)
    wm, wv = np.array([b * yb / c, b * ya / c]), np.full(2, c - b * b / c)
    assert np.max(np.abs(mean - wm)) <= 1e-12 and np.max(np.abs(var - wv)) <= 1e-12 * wv[0]
    wl = -0.5 * np.log(2 * np.pi * wv) - 0.5 * (np.array([ya, yb]) - wm) ** 2 / wv
    assert np.max(np.abs(lpd - wl)) <= 1e-12 and abs(tot - wl.sum()) <= 1e-12


SCHEDULES = [(3, 257), (30, 257), (50, 257), (512, 130)]   # latency, mid-size, throughput (fused diagonal), full batch


@pytest.fixture(scope="module")
def schedule_runs(engine):
    """One call per schedule; fit 1's window also sits in the last slot.  Shared by the tests below, never modified."""
    runs = {}
    for B, N in SCHEDULES:
        X, y, theta = problem(B, N, 3, 1, 7 + B)
        X[-1], y[-1], theta[-1] = X[1], y[1], theta[1]
        ctx = ctx_for(engine, B, N, 3)
        out = ctx.loo_batch(X, y, theta, 1)
        # the same call size with every other window replaced: new neighbours, other slot for the window of fit 1
        X2, y2, theta2 = problem(B, N, 3, 1, 1007 + B)
        X2[0], y2[0], theta2[0] = X[1], y[1], theta[1]
        out2 = ctx.loo_batch(X2, y2, theta2, 1)
        runs[B] = (X, y, theta, out, out2)
        ctx.close()
    return runs


@pytest.mark.parametrize("B,N", SCHEDULES)
def test_every_schedule_meets_the_oracle(schedule_runs, B, N):
    X, y, theta, out, _ = schedule_runs[B]
    assert out[0] == 0 and not out[6].any()
    for b in sorted({0, 1, 2, B // 2, B - 2, B - 1}):
        check_fit(out, b, 1, theta[b], X[b], y[b])
    assert np.all(np.isfinite(out[4]))


@pytest.mark.parametrize("B,N", SCHEDULES)
def test_outputs_do_not_depend_on_slot_or_neighbours(schedule_runs, B, N):
    _, _, _, out, out2 = schedule_runs[B]
    for u, w in zip(out[1:6], out2[1:6]):
        assert np.array_equal(u[1], u[B - 1]) and np.array_equal(u[1], w[0])


def test_single_call_is_the_batch_of_one_and_leaves_the_context_fitted(engine):
    N, d, kid = 257, 3, 3
    X, y, theta = problem(1, N, d, kid, 5)
    ctx = ctx_for(engine, 1, N, d)
    out = ctx.loo_batch(X, y, theta, kid)
    mean, var, lpd, tot = ctx.loo(X[0], y[0], kid, theta[0])
    assert np.array_equal(mean, out[1][0]) and np.array_equal(var, out[2][0]) and np.array_equal(lpd, out[3][0]) and tot == out[4][0]
    Xs = X[0][-20:] + 0.1
    pm, pv = ctx.predict(Xs)
    om, ov = lo.mo.predict(lo.mo.fit(kid, theta[0], X[0], y[0]), Xs)
    assert np.max(np.abs(pm - om)) <= TOL * np.max(np.abs(om)) and np.max(np.abs(pv - ov) / ov) <= TOL
    assert np.max(np.abs(ctx.alpha() - lo.fit(kid, theta[0], X[0], y[0]).alpha)) <= TOL * np.max(np.abs(ctx.alpha()))
    # short windows too (cgp_nll_grad would take the one-launch kernel there): the factor panel is resident
    Xs_, ys_, ths = problem(1, 40, 1, 2, 6)
    ctx.loo(Xs_[0], ys_[0], 2, ths[0])
    f = go.fit(2, ths[0], Xs_[0], ys_[0])
    assert np.max(np.abs(ctx.factor() - f.L)) <= TOL * np.max(np.abs(f.L))


def test_logml_is_the_marginal_calls(engine):
    B, N, d, kid = 4, 200, 2, 1
    X, y, theta = problem(B, N, d, kid, 12)
    ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)
    out = ctx.loo_batch(X, y, theta, kid)
    rc, _, _, logml, info = ctx.fit_predict_batch(X, y, X[:, :4], theta, kid)
    assert rc == 0 and out[0] == 0 and np.max(np.abs(out[5] - logml) / np.abs(logml)) <= 1e-9


def device_arrays(torch, X, y, theta):
    th = np.zeros((X.shape[0], 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, th)]


def device_outputs(torch, B, N):
    f = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    return f(B, N), f(B, N), f(B, N), f(B), f(B), torch.empty(B, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("B,N", [(3, 130), (50, 257)])
def test_host_device_and_graph_replay_agree_bitwise(engine, B, N):
    """The legacy stream, CGP_STREAM_CTX and a captured side stream against the host form."""
    import torch
    d, kid = 3, 1
    X, y, theta = problem(B, N, d, kid, 9 + B)
    ctx = ctx_for(engine, B, N, d)
    host = ctx.loo_batch(X, y, theta, kid)
    assert host[0] == 0
    dX, dy, dth = device_arrays(torch, X, y, theta)
    outs = device_outputs(torch, B, N)
    ptrs = [t.data_ptr() for t in outs]

    def clear():
        for t in outs[:5]:
            t.fill_(-1.0)
        outs[5].fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        for t, h in zip(outs[:5], host[1:6]):
            assert np.array_equal(t.cpu().numpy(), h)
        assert not outs[5].cpu().numpy().any()

    def enqueue(s):
        assert ctx.loo_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, *ptrs, stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    if B > 3:
        return
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()


def test_null_outputs_leave_the_others_unchanged(engine):
    """Each output alone gives the bits it has beside the others (lpd_sum without loo_lpd runs through the scratch copy)."""
    B, N, d, kid = 3, 130, 1, 2
    X, y, theta = problem(B, N, d, kid, 3)
    ctx = ctx_for(engine, B, N, d)
    full = ctx.loo_batch(X, y, theta, kid)
    lib, p, ip = ctx.lib, engine._p, engine._ip
    for k in range(4):
        bufs = [np.full((B, N), -1.0), np.full((B, N), -1.0), np.full((B, N), -1.0), np.full(B, -1.0)]
        args = [p(bufs[i]) if i == k else None for i in range(4)]
        assert lib.cgp_loo_batch(ctx.h, B, N, d, kid, p(X), p(y), p(theta), theta.shape[1], *args, None, None) == 0
        assert np.array_equal(bufs[k], full[1 + k])


def test_jitter_ladder_is_per_fit(engine):
    """test_gpu_joint_batch.py::test_jitter_ladder_is_per_fit_and_contracts_the_right_slab's input: fit 1 needs the first rung and
    is re-submitted as a call of one fit.  Its LOO meets the oracle at that jitter (which loo_var includes) at the bar; fits 0 and
    2 are bitwise what they are without the bad neighbour."""
    rng = np.random.default_rng(21)
    N, d, B = 200, 1, 3
    X = np.stack([np.sort(rng.normal(size=(N, d)), 0) for _ in range(B)])
    Xgood = X.copy()
    X[1, :, 0] = np.repeat(np.arange(N // 2, dtype=float), 2)         # duplicated inputs -> rank deficient K
    y, ygood = np.sin(X[:, :, 0]), np.sin(Xgood[:, :, 0])
    th = np.array([[1.0, 1.0, 0.05], [1.0, 3.0, -1e-8 - 2e-7], [1.0, 1.0, 0.05]])   # window 1: slightly indefinite
    thgood = np.array([[1.0, 1.0, 0.05]] * 3)
    want = lo.loo(0, th[1], X[1], y[1])
    assert want.jitter > 0
    ctx = ctx_for(engine, B, N, d)
    out = ctx.loo_batch(X, y, th, 0)
    assert out[0] == 0 and not out[6].any()
    print('fit 1 (jitter %.3g): errors' % want.jitter, lo.check((out[1][1], out[2][1], out[3][1], out[4][1]), want, y[1]))
    for b in (0, 2):
        check_fit(out, b, 0, th[b], X[b], y[b])
    good = ctx.loo_batch(Xgood, ygood, thgood, 0)
    assert good[0] == 0 and same(out, good, [0, 2])
    # the single call climbs the same ladder and reports the jitter
    mean, var, lpd, tot = ctx.loo(X[1], y[1], 0, th[1])
    assert np.array_equal(mean, out[1][1]) and np.array_equal(var, out[2][1]) and tot == out[4][1]
    assert abs(ctx.last_jitter() - want.jitter) <= 1e-12 * want.jitter


def test_fit_that_stays_indefinite_is_nan_neighbours_are_right(engine):
    """Host form: the ladder gives up on fit 1 (negative definite), the call returns its status; device form: no ladder."""
    import torch
    B, N, d, kid = 3, 200, 2, 1
    X, y, theta = problem(B, N, d, kid, 8)
    theta[1, -1] = -2.0 * theta[1, 0]
    ctx = ctx_for(engine, B, N, d)
    out = ctx.loo_batch(X, y, theta, kid)
    assert out[0] > 0 and out[6][1] == out[0] and out[6][0] == 0 and out[6][2] == 0
    assert all(np.all(np.isnan(a[1])) for a in out[1:5])
    for b in (0, 2):
        check_fit(out, b, kid, theta[b], X[b], y[b])
    with pytest.raises(engine.CgpError):
        ctx.loo(X[1], y[1], kid, theta[1])
    with pytest.raises(engine.CgpError):
        ctx.predict(X[1][:3])   # not fitted
    dX, dy, dth = device_arrays(torch, X, y, theta)
    outs = device_outputs(torch, B, N)
    assert ctx.loo_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, *[t.data_ptr() for t in outs]) == 0
    torch.cuda.synchronize()
    dev = [None] + [t.cpu().numpy() for t in outs]
    assert dev[6][1] > 0 and dev[6][0] == 0 and dev[6][2] == 0
    assert all(np.all(np.isnan(a[1])) for a in dev[1:5])
    assert same(dev, out, [0, 2])


def test_argument_state_and_capacity_errors(engine):
    ctx = engine.Context(max_n=16, max_m=16, max_d=1, max_batch=2)
    buf = np.zeros(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib

    def one(h=ctx.h, X=p, N=8, d=1, kid=2, th=p, outs=(p, p, p, p)):
        return lib.cgp_loo(h, X, p, N, d, kid, th, *outs)

    def bat(h=ctx.h, B=1, N=8, d=1, kid=2, X=p, stride=4, outs=(p, p, p, p)):
        return lib.cgp_loo_batch(h, B, N, d, kid, X, p, p, stride, *outs, p, ip)

    def dev(h=ctx.h, B=1, N=8, d=1, kid=2, X=a, lm=a, info=a, outs=(a, a, a, a)):
        return lib.cgp_loo_batch_device(h, B, N, d, kid, X, a, a, None, *outs, lm, info, None)

    for f in (one, bat, dev):
        assert f(h=None) == EINVAL
        assert f(N=0) == EINVAL and f(d=0) == EINVAL and f(kid=5) == EINVAL and f(kid=-1) == EINVAL
        assert f(kid=2, d=2) == EINVAL   # RBF x Brownian is one-dimensional
        assert f(N=17) == ECAPACITY and f(kid=1, d=2) == ECAPACITY
        assert f(X=None) == EINVAL
        assert f(outs=(None,) * 4) == EINVAL
    assert bat(B=0) == EINVAL and dev(B=0) == EINVAL and bat(B=3) == ECAPACITY and dev(B=3) == ECAPACITY
    assert bat(stride=3) == EINVAL and one(th=None) == EINVAL
    assert dev(lm=None) == EINVAL and dev(info=None) == EINVAL
    small_m = engine.Context(max_n=16, max_m=4, max_d=1, max_batch=1)   # needs max_m >= N, as cgp_nll_grad does
    assert one(h=small_m.h) == ECAPACITY and bat(h=small_m.h) == ECAPACITY and dev(h=small_m.h) == ECAPACITY
    # the context is still usable
    X, y, theta = problem(1, 8, 1, 2, 1)
    assert np.all(np.isfinite(ctx.loo(X[0], y[0], 2, theta[0])[0]))


def test_fp32_contexts_are_refused_and_stay_usable(engine):
    ctx = engine.Context(max_n=64, max_m=64, max_d=2, max_batch=2, dtype=F32)
    X, y, theta = problem(2, 64, 2, 1, 4)
    p = engine._p
    buf = np.zeros(2 * 64)
    assert ctx.lib.cgp_loo(ctx.h, p(X[0]), p(y[0]), 64, 2, 1, p(theta[0]), p(buf), p(buf), p(buf), p(buf)) == EINVAL
    assert ctx.lib.cgp_loo_batch(ctx.h, 2, 64, 2, 1, p(X), p(y), p(theta), 4, p(buf), p(buf), p(buf), p(buf), None, None) == EINVAL
    a = buf.ctypes.data
    assert ctx.lib.cgp_loo_batch_device(ctx.h, 2, 64, 2, 1, a, a, a, None, a, a, a, a, a, a, None) == EINVAL
    rc, logml = ctx.fit(X[0], y[0], 1, theta[0])
    assert rc == 0 and np.isfinite(logml)


def test_symbols_present(engine):
    lib = engine.load()
    for name in ("cgp_loo", "cgp_loo_batch", "cgp_loo_batch_device", "cgp_window_loo", "cgp_window_loo_device"):
        assert hasattr(lib, name) and name in engine.EXPORTS
