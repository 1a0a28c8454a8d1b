"""GPU parity of the sliding windows' joint forecast (cgp_window_predict_cov: mean and the full posterior covariance at M test
points; cgp_window_sample: sample paths from it) against the oracle, which refits the window's samples from scratch."""
import numpy as np
import pytest

from oracle import gp_oracle as go
from joint_oracle import sliding_window_joint, sample_matrix, sample_paths
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h


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
    return {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]),
            1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]


def points_for(kid, X, t, M, rng):
    """RBF x Brownian: the reference's grid (the ticks after the last sample); SE: points around the window's inputs."""
    if kid == 2:
        return X[t - 1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    lo = max(0, t - 50)
    return X[rng.integers(lo, max(t, 1), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def close(mean, cov, omu, ocov, tol=TOL):
    """The mean against the oracle's largest mean, every covariance entry against sqrt(cov_ii cov_jj) (its natural scale)."""
    assert np.max(np.abs(mean - omu)) <= tol * max(np.max(np.abs(omu)), 1e-12), np.max(np.abs(mean - omu))
    sd = np.sqrt(np.diag(ocov))
    assert np.max(np.abs(cov - ocov) / np.outer(sd, sd)) < tol, np.max(np.abs(cov - ocov) / np.outer(sd, sd))
    assert np.max(np.abs(np.diag(cov) - np.diag(ocov)) / np.diag(ocov)) < tol


def ctx_with(engine, W, N, d, kid, theta, max_m):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    assert ctx.window_joint_reserve(max_m) == 0
    return ctx


@pytest.mark.parametrize("kid,N,d", [(2, 16, 1), (2, 40, 1), (0, 33, 2), (1, 64, 3), (0, 50, 4), (1, 45, 5), (1, 100, 6)])
def test_joint_forecast_matches_refit_oracle(engine, kid, N, d):
    """M = 1, 17, 100 (and 599 once) at several moments of one stream: empty, filling, full, either side of the ring's
    compaction, after the window has turned over.  Symmetric exactly; mean / diagonal are cgp_window_predict's; noise touches
    the diagonal only."""
    T = 3 * N + 6
    X, y = stream(T, d, 100 + N)
    theta = theta_of(kid, d)
    rng = np.random.default_rng(N)
    ctx = ctx_with(engine, 1, N, d, kid, theta, 599)
    fed = 0
    for t in (0, 1, N // 2, N, 2 * N - 1, 2 * N, 2 * N + 1, T):
        if t > fed:
            ctx.window_push(X[fed:t][None], y[fed:t][None])
            fed = t
        for M in (1, 17, 100) + ((599,) if t == T else ()):
            Xs = points_for(kid, X, max(t, 1), M, rng)
            covs = {}
            for noise in (True, False):
                mean, cov = ctx.window_predict_cov(Xs, include_noise=noise)
                assert mean.shape == (1, M) and cov.shape == (1, M, M)
                assert np.array_equal(cov[0], cov[0].T)
                pm, pv = ctx.window_predict(Xs, include_noise=noise)
                assert np.array_equal(pm, mean) and np.array_equal(pv[0], np.diag(cov[0]))
                omu, ocov = sliding_window_joint(kid, theta, N, X[:t], y[:t], Xs, include_noise=noise)
                if t == 0:
                    assert np.all(mean == 0.0)
                    np.testing.assert_allclose(cov[0], ocov, rtol=1e-12, atol=1e-300)
                else:
                    close(mean[0], cov[0], omu, ocov)
                covs[noise] = cov[0]
            diff = covs[True] - covs[False]
            assert np.array_equal(diff - np.diag(np.diag(diff)), np.zeros((M, M)))
            np.testing.assert_allclose(np.diag(diff), go.noise_var(kid, theta), rtol=1e-6)


def test_after_two_thousand_ticks(engine):
    N, d, T, M = 64, 3, 2000, 100
    X, y = stream(T, d, 2000)
    theta = theta_of(1, d)
    ctx = ctx_with(engine, 1, N, d, 1, theta, M)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, np.random.default_rng(1))
    mean, cov = ctx.window_predict_cov(Xs)
    close(mean[0], cov[0], *sliding_window_joint(1, theta, N, X, y, Xs))


def test_config4_window512_horizon599(engine):
    """configs[3] size: N = 512, d = 3 after 1 200 ticks, M = 599; the covariance of well-separated points is positive
    semi-definite to rounding."""
    N, d, T, M = 512, 3, 1200, 599
    X, y = stream(T, d, 7)
    theta = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])
    ctx = ctx_with(engine, 1, N, d, 1, theta, M)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, np.random.default_rng(5))
    mean, cov = ctx.window_predict_cov(Xs, include_noise=False)
    omu, ocov = sliding_window_joint(1, theta, N, X, y, Xs, include_noise=False)
    close(mean[0], cov[0], omu, ocov)
    assert np.linalg.eigvalsh(cov[0])[0] >= -1e-9 * np.max(np.diag(cov[0]))


def test_joint_forecast_does_not_touch_the_windows(engine):
    """push A, joint forecasts, push B = push A, push B on a second context, bitwise; window_predict / window_nll_grad after
    them are unchanged."""
    N, d, T = 48, 2, 170
    X, y = stream(T, d, 77)
    theta = theta_of(1, d)
    rng = np.random.default_rng(1)
    Xs = points_for(1, X, T, 70, rng)
    xi = rng.normal(size=(1, 5, 70))
    outs = []
    for between in (True, False):
        ctx = ctx_with(engine, 1, N, d, 1, theta, 70)
        ctx.window_push(X[:90][None], y[:90][None])
        if between:
            ctx.window_predict_cov(Xs)
            ctx.window_sample(Xs, xi)
            ctx.window_predict_cov(Xs[:3], include_noise=False)
        outs.append(ctx.window_push(X[90:][None], y[90:][None]) + ctx.window_predict(Xs) + ctx.window_nll_grad())
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def many_windows(W, N, d, T, M, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + T, dtype=np.float64)
    X = np.empty((W, T, d))
    X[:, :, 0] = (t - t.mean()) / t.std()
    X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
    y = np.stack([synth._slip_series(rng, t) for _ in range(W)])
    theta = np.column_stack([0.02 + 0.01 * rng.random(W)] + [0.8 + rng.random(W) for _ in range(d)] + [1e-3 * (1 + rng.random(W))])
    Xs = X[:, rng.integers(T - N, T, size=M)] + 0.3 * rng.normal(size=(W, M, d))
    return X, y, theta, Xs, rng


def test_many_windows_are_independent_of_slot_and_neighbours(engine):
    """600 windows x N = 64, M = 100, S = 3: some against the oracle; a window's covariance and paths bitwise equal to the same
    stream in a context of one and of two windows."""
    W, N, d, T, M, S = 600, 64, 2, 150, 100, 3
    X, y, theta, Xs, rng = many_windows(W, N, d, T, M, 600)
    xi = rng.normal(size=(W, S, M))
    ctx = ctx_with(engine, W, N, d, 1, theta, M)
    ctx.window_push(X, y)
    mean, cov = ctx.window_predict_cov(Xs)
    paths, info = ctx.window_sample(Xs, xi, include_noise=True)
    assert not info.any()
    for w in (0, 85, 299, 300, 599):
        omu, ocov = sliding_window_joint(1, theta[w], N, X[w], y[w], Xs[w])
        close(mean[w], cov[w], omu, ocov)
        op = sample_paths(omu, ocov, 0.0, 1e-6, xi[w])
        assert np.max(np.abs(paths[w] - op)) <= TOL * np.max(np.abs(op))
    for ws in ([299], [513, 7]):
        big = ctx_with(engine, W, N, d, 1, theta, M)
        small = ctx_with(engine, len(ws), N, d, 1, theta[ws], M + 30)   # another reservation: the scratch's strides differ
        for k in range(40):   # one-tick pushes are the same kernel whatever the context (test_gpu_window_forecast.py)
            big.window_push(X[:, k:k + 1], y[:, k:k + 1])
            small.window_push(X[ws, k:k + 1], y[ws, k:k + 1])
        bm, bc = big.window_predict_cov(Xs)
        sm, sc = small.window_predict_cov(Xs[ws])
        assert np.array_equal(bm[ws], sm) and np.array_equal(bc[ws], sc)
        bp, _ = big.window_sample(Xs, xi)
        sp, _ = small.window_sample(Xs[ws], xi[ws])
        assert np.array_equal(bp[ws], sp)


def test_host_device_and_graph_replay_agree_bitwise(engine):
    import torch
    W, N, d, T, M, S = 3, 40, 3, 100, 53, 7
    rng = np.random.default_rng(9)
    Xw, yw = zip(*[stream(T, d, 500 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = theta_of(1, d)
    Xs = X[:, rng.integers(T - N, T, size=M)] + 0.2 * rng.normal(size=(W, M, d))
    xi = rng.normal(size=(W, S, M))
    ctx = ctx_with(engine, W, N, d, 1, theta, 64)
    ctx.window_push(X, y)
    mean, cov = ctx.window_predict_cov(Xs)
    paths, info = ctx.window_sample(Xs, xi, include_noise=True, jitter_rel=1e-8)
    dxs, dxi = torch.from_numpy(Xs).cuda(), torch.from_numpy(xi).cuda()
    dm = torch.empty((W, M), dtype=torch.float64, device="cuda")
    dc = torch.empty((W, M, M), dtype=torch.float64, device="cuda")
    dp = torch.empty((W, S, M), dtype=torch.float64, device="cuda")
    di = torch.empty(W, dtype=torch.int32, device="cuda")

    def clear():
        for t in (dm, dc, dp):
            t.fill_(-1.0)
        di.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dc.cpu().numpy(), cov)
        assert np.array_equal(dp.cpu().numpy(), paths) and not di.cpu().numpy().any()

    def enqueue(s):
        assert ctx.window_predict_cov_device(M, dxs.data_ptr(), True, dm.data_ptr(), dc.data_ptr(), stream=s) == 0
        assert ctx.window_sample_device(M, dxs.data_ptr(), S, dxi.data_ptr(), True, 1e-8, dp.data_ptr(), di.data_ptr(), stream=s) == 0

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


@pytest.mark.parametrize("kid,N,d,M", [(1, 64, 3, 45), (2, 40, 1, 100), (0, 33, 2, 16), (0, 33, 2, 520)])   # M = 520: eight tiles per wave
def test_paths_factor_and_random_draws(engine, kid, N, d, M):
    """xi = unit vectors returns C: lower triangular, C C^T = the oracle's matrix (cov + noise + jitter) to 1e-9; random xi
    against sample_paths, S = 1 and S = 50."""
    T = 2 * N + 9
    X, y = stream(T, d, 31 + N)
    theta = theta_of(kid, d)
    rng = np.random.default_rng(M)
    ctx = ctx_with(engine, 1, N, d, kid, theta, M)
    ctx.window_push(X[None], y[None])
    Xs = points_for(kid, X, T, M, rng)
    for noise in (False, True):
        mean, cov = ctx.window_predict_cov(Xs, include_noise=False)
        sn = go.noise_var(kid, theta) if noise else 0.0
        out, info = ctx.window_sample(Xs, np.eye(M)[None], include_noise=noise, jitter_rel=1e-6)
        assert info[0] == 0
        C = (out[0] - mean[0][None, :]).T   # path s = mean + column s of C
        assert np.array_equal(np.triu(C, 1), np.zeros((M, M)))
        omu, ocov = sliding_window_joint(kid, theta, N, X, y, Xs, include_noise=False)
        A = sample_matrix(ocov, sn, 1e-6)
        # the factor of a nearly singular matrix is not determined to 1e-9, its square is; the device's own covariance is the
        # matrix it factored, the oracle's differs from it by the parity bar
        Ad = sample_matrix(cov[0], sn, 1e-6)
        assert np.max(np.abs(C @ C.T - Ad)) <= 1e-9 * np.max(np.diag(Ad))
        assert np.max(np.abs(C @ C.T - A)) <= TOL * np.max(np.diag(A))
        for S in (1, 50):
            xi = rng.normal(size=(1, S, M))
            out, info = ctx.window_sample(Xs, xi, include_noise=noise, jitter_rel=1e-6)
            dev = mean[0][None, :] + xi[0] @ C.T
            assert out.shape == (1, S, M) and np.max(np.abs(out[0] - dev)) <= 1e-12 * np.max(np.abs(dev))
            if noise:   # well conditioned: the factor itself is in parity
                op = sample_paths(omu, ocov, sn, 1e-6, xi[0])
                assert np.max(np.abs(out[0] - op)) <= TOL * np.max(np.abs(op))


def test_rank_deficient_request_is_reported_not_fatal(engine):
    """Half of window 1's test points are copies of one point: without jitter and noise its matrix is singular (pivots of
    rounding size, either sign) -- an arithmetic outcome, reported in info with NaN paths; the other windows' paths are right;
    with jitter_rel = 1e-6 the same request succeeds."""
    W, N, d, T, M, S = 3, 32, 2, 70, 20, 4
    X, y, theta, Xs, rng = many_windows(W, N, d, T, M, 33)
    Xs = Xs + 2.0 * rng.normal(size=Xs.shape)   # spread out: the other windows' matrices are comfortably positive definite
    Xs[1, 10:] = Xs[1, 4]
    xi = rng.normal(size=(W, S, M))
    ctx = ctx_with(engine, W, N, d, 1, theta, M)
    ctx.window_push(X, y)
    out, info, rc = ctx.window_sample(Xs, xi, include_noise=False, jitter_rel=0.0, check=False)
    assert rc == 2 and info[0] == 0 and info[2] == 0 and 11 <= info[1] <= M
    assert np.all(np.isnan(out[1]))
    with pytest.raises(engine.CgpError):
        ctx.window_sample(Xs, xi, include_noise=False, jitter_rel=0.0)
    for w in (0, 2):
        omu, ocov = sliding_window_joint(1, theta[w], N, X[w], y[w], Xs[w], include_noise=False)
        op = sample_paths(omu, ocov, 0.0, 0.0, xi[w])
        assert np.max(np.abs(out[w] - op)) <= TOL * np.max(np.abs(op))
    out, info = ctx.window_sample(Xs, xi, include_noise=False, jitter_rel=1e-6)
    assert not info.any() and np.all(np.isfinite(out))


def test_empty_failed_and_retuned_windows(engine):
    """Empty windows answer with the prior; a failed window with NaN while the others are unaffected; after set_theta the joint
    forecast follows the new theta."""
    W, N, d, T, M = 3, 24, 1, 30, 40
    Xw, yw = zip(*[stream(T, d, 900 + w) for w in range(W)])
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(theta_of(0, d), (W, 1))
    theta[1, -1] = -2.0 * theta[1, 0]
    rng = np.random.default_rng(2)
    Xs = X[:, -1:, :] + rng.random((W, M, 1)) * 5.0
    ctx = ctx_with(engine, W, N, d, 0, theta, M)
    mean, cov = ctx.window_predict_cov(Xs, include_noise=False)
    for w in (0, 2):
        assert np.all(mean[w] == 0.0)
        np.testing.assert_allclose(cov[w], go.kernel_K(0, theta[w], Xs[w]), rtol=1e-12, atol=1e-300)
    with pytest.raises(engine.CgpError):
        ctx.window_push(X, y)
    code = ctx.window_state(1)[1]
    mean, cov, rc = ctx.window_predict_cov(Xs, check=False)
    assert rc == code > 0
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(cov[1]))
    out, info, rc = ctx.window_sample(Xs, rng.normal(size=(W, 2, M)), include_noise=True, check=False)
    assert rc == 2 and info[1] > 0 and np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))
    for w in (0, 2):
        close(mean[w], cov[w], *sliding_window_joint(0, theta[w], N, X[w], y[w], Xs[w]))
    new = np.tile(np.array([0.05, 2.0, 2e-3]), (W, 1))
    ctx.window_set_theta(new)   # revives window 1 as well
    mean, cov = ctx.window_predict_cov(Xs)
    for w in range(W):
        close(mean[w], cov[w], *sliding_window_joint(0, new[w], N, X[w], y[w], Xs[w]))


@pytest.mark.parametrize("N,T,M", [(1024, 1100, 70), (1536, 1700, 40)])
def test_long_window_forms(engine, N, T, M):
    """The one-tile and the half-tile form of the solve (correct, not tuned)."""
    d = 2
    X, y = stream(T, d, N)
    theta = theta_of(1, d)
    rng = np.random.default_rng(3)
    ctx = ctx_with(engine, 1, N, d, 1, theta, M)
    ctx.window_push(X[None], y[None])
    Xs = points_for(1, X, T, M, rng)
    mean, cov = ctx.window_predict_cov(Xs)
    omu, ocov = sliding_window_joint(1, theta, N, X, y, Xs)
    close(mean[0], cov[0], omu, ocov)
    xi = rng.normal(size=(1, 3, M))
    out, _ = ctx.window_sample(Xs, xi, include_noise=True)
    op = sample_paths(omu, ocov, 0.0, 1e-6, xi[0])
    assert np.max(np.abs(out[0] - op)) <= TOL * np.max(np.abs(op))


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    buf = np.zeros(64)
    ib = np.zeros(4, dtype=np.int32)
    p, a = engine._p(buf), buf.ctypes.data
    lib = ctx.lib
    assert lib.cgp_window_joint_reserve(ctx.h, 8) == ESTATE
    assert lib.cgp_window_predict_cov(ctx.h, 1, p, 1, p, p) == ESTATE
    ctx.window_init(1, 8, 1, 2, theta_of(2, 1))
    assert lib.cgp_window_predict_cov(ctx.h, 1, p, 1, p, p) == ESTATE      # no reservation yet
    assert lib.cgp_window_sample(ctx.h, 1, p, 1, p, 0, 1e-6, p, None) == ESTATE
    assert lib.cgp_window_predict_cov_device(ctx.h, 1, a, 1, a, a, None) == ESTATE
    assert lib.cgp_window_sample_device(ctx.h, 1, a, 1, a, 0, 1e-6, a, None, None) == ESTATE
    assert lib.cgp_window_joint_reserve(ctx.h, 0) == EINVAL and lib.cgp_window_joint_reserve(ctx.h, 1025) == EINVAL
    assert lib.cgp_window_joint_reserve(ctx.h, 4) == 0
    assert lib.cgp_window_predict_cov(ctx.h, 5, p, 1, p, p) == ECAPACITY
    assert lib.cgp_window_sample(ctx.h, 5, p, 1, p, 0, 1e-6, p, None) == ECAPACITY
    assert lib.cgp_window_predict_cov(ctx.h, 0, p, 1, p, p) == EINVAL
    assert lib.cgp_window_predict_cov(ctx.h, 1, None, 1, p, p) == EINVAL
    assert lib.cgp_window_predict_cov(ctx.h, 1, p, 1, p, None) == EINVAL
    assert lib.cgp_window_predict_cov_device(ctx.h, 1, a, 1, None, a, None) == EINVAL
    assert lib.cgp_window_sample(ctx.h, 0, p, 1, p, 0, 1e-6, p, None) == EINVAL
    assert lib.cgp_window_sample(ctx.h, 1, p, 0, p, 0, 1e-6, p, None) == EINVAL
    assert lib.cgp_window_sample(ctx.h, 1, p, 1, None, 0, 1e-6, p, None) == EINVAL
    assert lib.cgp_window_sample(ctx.h, 1, p, 1, p, 0, -1e-6, p, None) == EINVAL
    assert lib.cgp_window_sample(ctx.h, 1, p, 1, p, 0, float("nan"), p, None) == EINVAL
    assert lib.cgp_window_sample_device(ctx.h, 1, a, 1, a, 0, 1e-6, None, None, None) == EINVAL
    buf[:2] = 3.0, 4.5
    assert lib.cgp_window_sample(ctx.h, 2, p, 1, p, 1, 1e-6, engine._p(np.zeros(2)), ib.ctypes.data_as(engine._ip)) == 0 and ib[0] == 0
    ctx.window_init(1, 8, 1, 2, theta_of(2, 1))                            # a new init drops the reservation
    assert lib.cgp_window_predict_cov(ctx.h, 1, p, 1, p, p) == ESTATE


def test_paths_feed_the_stop_time_lookahead(engine):
    """The ensemble member that draws its own slip curve: 64 paths of one window's 599-tick forecast into
    cgp_predict_stop_batch with mean = path, sigma = 0; every member's result equals the oracle's look-ahead on the same path."""
    N, M, S = 149, 599, 64
    theta = theta_of(2, 1)
    tw, sw = synth.reference_window(n=200, tick0=11, seed=4000)
    X, y = tw[None, :, None], sw[None]
    ctx = ctx_with(engine, 1, N, 1, 2, theta, M)
    ctx.window_push(X, y)
    Xs = X[:, -1:, :] + 1.0 + np.arange(M, dtype=np.float64)[None, :, None]
    xi = np.random.default_rng(64).normal(size=(1, S, M))
    paths, info = ctx.window_sample(Xs, xi, include_noise=False, jitter_rel=1e-6)
    assert info[0] == 0
    omu, ocov = sliding_window_joint(2, theta, N, X[0], y[0], Xs[0], include_noise=False)
    sd = np.sqrt(np.diag(ocov))
    assert np.max(np.abs(paths[0].mean(0) - omu) / sd) < 1.0   # 64 draws: the ensemble mean within a few standard errors
    p = paths[0]
    st = synth.filter_state(2000)
    P, Q, STM, Hv, pos = (np.stack([st[j]] * S) for j in range(5))
    fired, cmd, iout, xy = ctx.predict_stop_batch(p, np.zeros_like(p), P, Q, STM, Hv, pos, 50.0, 50.2)
    for s in range(S):
        ef, ec, ei, exy = go.predict_stop(p[s], np.zeros(M), P[s], Q[s], STM[s], go.unpack_H(Hv[s], True), pos[s], 50.0, 50.2)
        assert bool(fired[s]) == ef and iout[s] == ei
        assert cmd[s] == pytest.approx(ec, rel=1e-12) and xy[s] == pytest.approx(exy, rel=1e-6)
    # the members are distinct realisations (tick-to-tick correlated: neighbouring ticks move together); the reference's
    # look-ahead sees slip only through the spread of its three sigma points, which sigma = 0 puts at the floor of R, so here the
    # members' stop times coincide -- what is checked is that every member's path goes through the look-ahead unchanged
    dev = p - p.mean(0)
    assert np.min(dev.std(0)[1:]) > 0.0
    assert np.mean(dev[:, 1:] * dev[:, :-1]) > 0.5 * np.mean(dev * dev)
