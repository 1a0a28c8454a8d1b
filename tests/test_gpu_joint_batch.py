"""GPU parity of the joint forecast after batch / single fits (cgp_fit_predict_cov_batch[_device]: mean and the full posterior
covariance at M test points; cgp_fit_sample_batch[_device]: sample paths from it; cgp_predict_cov / cgp_sample after a single
fit) against the refit oracle, through the C ABI.  Bar: the project's fp64 bar, 1e-6, in the metric of
test_gpu_window_joint.py::close (the same formula in 80-bit arithmetic differs from the fp64 oracle by <= 6.3e-13 in it)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
from joint_oracle import sliding_window_joint, sample_matrix, sample_paths
import matern_oracle as mo
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


def noise_of(kid, theta):
    return float(theta[-1]) if kid >= 3 else go.noise_var(kid, theta)


def window(N, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)]), y


def points_for(kid, X, M, rng):
    """RBF x Brownian: the reference's grid (the ticks after the last sample); else points around the window's last inputs."""
    if kid == 2:
        return X[-1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    N = len(X)
    return X[rng.integers(max(0, N - 50), N, size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def problem(B, N, d, M, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, yw = zip(*[window(N, d, seed + 17 * b, tick0=11 + b) for b in range(B)])
    X, y = np.stack(Xw), np.stack(yw)
    Xs = np.stack([points_for(kid, X[b], M, rng) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return X, y, Xs, theta, rng


def oracle_joint(kid, theta, X, y, Xs, noise=True):
    """Refit from scratch (GPy's jitter ladder included): mean (M,), cov (M, M)."""
    if kid >= 3:
        return mo.predict_cov(mo.fit(kid, theta, X, y), Xs, noise)
    return sliding_window_joint(kid, theta, len(y), X, y, Xs, include_noise=noise)


def close(mean, cov, omu, ocov, tol=TOL):
    """The mean against the oracle's largest mean, every covariance entry against sqrt(cov_ii cov_jj) (its natural scale)."""
    em = np.max(np.abs(mean - omu)) / max(np.max(np.abs(omu)), 1e-12)
    sd = np.sqrt(np.diag(ocov))
    ec = np.max(np.abs(cov - ocov) / np.outer(sd, sd))
    ed = np.max(np.abs(np.diag(cov) - np.diag(ocov)) / np.diag(ocov))
    print(f"errors / bar: mean {em / tol:.3g} cov {ec / tol:.3g} diag {ed / tol:.3g}")
    assert em <= tol and ec < tol and ed < tol, (em, ec, ed)


def ctx_for(engine, B, N, d, M, reserve_m=None, reserve_b=None):
    ctx = engine.Context(max_n=N, max_m=max(M, reserve_m or 0), max_d=d, max_batch=B)
    assert ctx.joint_reserve(reserve_b or B, reserve_m or M) == 0
    return ctx


GOLDEN = [("sk_se_iso_n256_d3", 100), ("sk_se_ard_n134_d6", 17), ("sk_se_ard_n2048_d6", 599), ("mp_rbfbrownian_n134", 599),
          ("matern_sk_m32_n256_d3", 128), ("matern_sk_m52_n256_d3", 100), ("matern_sk_m52_n2048_d6", 599)]


@pytest.mark.parametrize("name,M", GOLDEN)
def test_golden_windows_every_kernel(engine, name, M):
    """The fixtures' windows and theta, test points around the inputs; noise on and off differ on the diagonal only; symmetric
    exactly; the single-fit calls are bitwise cgp_predict."""
    g = load_golden(name)
    X, y, theta, kid = g["X"], g["y"], g["theta"], int(g["kernel_id"])
    X = X[:, None] if X.ndim == 1 else X
    N, d = X.shape
    rng = np.random.default_rng(N + M)
    Xs = points_for(kid, X, M, rng)
    ctx = ctx_for(engine, 1, N, d, M)
    covs = {}
    for noise in (True, False):
        rc, mean, cov, logml, info = ctx.fit_predict_cov_batch(X[None], y[None], Xs[None], theta[None], kid, include_noise=noise)
        assert rc == 0 and info[0] == 0 and cov.shape == (1, M, M)
        assert np.array_equal(cov[0], cov[0].T)
        omu, ocov = oracle_joint(kid, theta, X, y, Xs, noise)
        close(mean[0], cov[0], omu, ocov)
        assert abs(logml[0] - float(g["logml"])) <= TOL * abs(float(g["logml"]))
        covs[noise] = cov[0]
    diff = covs[True] - covs[False]
    assert np.array_equal(diff - np.diag(np.diag(diff)), np.zeros((M, M)))
    np.testing.assert_allclose(np.diag(diff), noise_of(kid, theta), rtol=1e-6)
    assert ctx.fit(X, y, kid, theta)[0] == 0
    pm, pv = ctx.predict(Xs, include_noise=True)
    sm, sc = ctx.predict_cov(Xs, include_noise=True)
    assert np.array_equal(pm, sm) and np.array_equal(pv, np.diag(sc)) and np.array_equal(sc, sc.T)
    close(sm, sc, *oracle_joint(kid, theta, X, y, Xs, True))
    xi = rng.normal(size=(3, M))
    paths, pivot = ctx.sample(Xs, xi, include_noise=True, jitter_rel=1e-6)   # with noise: a well-conditioned factor
    assert pivot == 0
    lmu, lcov = oracle_joint(kid, theta, X, y, Xs, False)
    op = sample_paths(lmu, lcov, noise_of(kid, theta), 1e-6, xi)
    assert np.max(np.abs(paths - op)) <= TOL * np.max(np.abs(op))
    paths, pivot = ctx.sample(Xs, xi, include_noise=False, jitter_rel=1e-6)
    assert pivot == 0 and np.all(np.isfinite(paths))


@pytest.mark.parametrize("B", [1, 3, 40, 64, 200, 512])
def test_every_schedule(engine, B):
    """N = 300, d = 3, M = 70 through the latency, mid-size, fused and split schedules: some fits against the oracle, mean and
    diag(cov) bitwise the marginal call's mean / var (a tiled shape)."""
    N, d, M, kid, S = 300, 3, 70, 1, 5
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 1000 + B)
    xi = rng.normal(size=(B, S, M))
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, cov, logml, info = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid)
    assert rc == 0 and not info.any()
    rc, pm, pv, plm, _ = ctx.fit_predict_batch(X, y, Xs, theta, kid)
    assert np.array_equal(mean, pm) and np.array_equal(np.diagonal(cov, axis1=1, axis2=2), pv) and np.array_equal(logml, plm)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    rc, paths, _, _, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=True)
    assert rc == 0 and not sinfo.any()
    for b in sorted({0, B // 2, B - 1}):
        omu, ocov = oracle_joint(kid, theta[b], X[b], y[b], Xs[b])
        close(mean[b], cov[b], omu, ocov)
        lat = ocov - go.noise_var(kid, theta[b]) * np.eye(M)
        op = sample_paths(omu, lat, go.noise_var(kid, theta[b]), 1e-6, xi[b])
        assert np.max(np.abs(paths[b] - op)) <= TOL * np.max(np.abs(op))


def test_fit_is_independent_of_slot_neighbours_and_call_size(engine):
    """Fit 137 of a 200-fit call, alone, and as fit 2 of a 3-fit call (another reservation: the scratch's strides differ):
    covariance and paths bitwise (the header's fp64 promise, extended).  The joint calls run the schedule the marginal call of
    the same size runs, and mean / variance are bitwise that call's; so the promise is the marginal call's own: it holds among
    the mid-size and fused schedules, and N = 2700 is a window for which a lone fit takes them too (the latency schedule stops
    at N = 2560).  Inside the latency schedule's range: the next test."""
    N, d, M, kid, S, B = 2700, 3, 70, 1, 4, 200
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 77)
    xi = rng.normal(size=(B, S, M))
    big = ctx_for(engine, B, N, d, M)
    rc, bm, bc, _, _ = big.fit_predict_cov_batch(X, y, Xs, theta, kid)
    rc2, bp, _, _, _ = big.fit_sample_batch(X, y, Xs, theta, kid, xi)
    assert rc == 0 and rc2 == 0
    close(bm[137], bc[137], *oracle_joint(kid, theta[137], X[137], y[137], Xs[137]))
    for sel in ([137], [5, 190, 137]):
        small = ctx_for(engine, len(sel), N, d, M, reserve_m=M + 30)
        _, sm, sc, _, _ = small.fit_predict_cov_batch(X[sel], y[sel], Xs[sel], theta[sel], kid)
        _, sp, _, _, _ = small.fit_sample_batch(X[sel], y[sel], Xs[sel], theta[sel], kid, xi[sel])
        assert np.array_equal(bm[sel], sm) and np.array_equal(bc[sel], sc) and np.array_equal(bp[sel], sp)


def test_latency_range_calls_agree_with_larger_ones_to_rounding(engine):
    """N = 300: a lone fit and a 3-fit call take the latency schedule (a tile's inner dimension summed in ranges), a 200-fit call
    the fused one -- two summation orders of the same fp64 sums.  Slot and neighbours never matter (bitwise); across the two
    schedules the joint outputs agree as the marginal call's do: to 1e-9, the figure test_gpu_parity.py::
    test_config2_bench_batch_schedule holds two schedules' mean / variance to."""
    N, d, M, kid, S, B = 300, 3, 70, 1, 4, 200
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 78)
    xi = rng.normal(size=(B, S, M))
    big = ctx_for(engine, B, N, d, M)
    _, bm, bc, _, _ = big.fit_predict_cov_batch(X, y, Xs, theta, kid)
    _, bp, _, _, _ = big.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=True)
    outs = []
    for sel in ([137], [5, 190, 137]):
        small = ctx_for(engine, len(sel), N, d, M, reserve_m=M + 30)
        _, sm, sc, _, _ = small.fit_predict_cov_batch(X[sel], y[sel], Xs[sel], theta[sel], kid)
        _, sp, _, _, _ = small.fit_sample_batch(X[sel], y[sel], Xs[sel], theta[sel], kid, xi[sel], include_noise=True)
        outs.append((sm[-1], sc[-1], sp[-1]))
        sd = np.sqrt(np.diag(bc[137]))
        assert np.max(np.abs(sm[-1] - bm[137])) <= 1e-9 * np.max(np.abs(bm[137]))
        assert np.max(np.abs(sc[-1] - bc[137]) / np.outer(sd, sd)) <= 1e-9
        assert np.max(np.abs(sp[-1] - bp[137])) <= 1e-9 * np.max(np.abs(bp[137]))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kid,N,d", [(0, 100, 2), (2, 100, 1), (1, 16, 3), (4, 100, 3), (1, 9, 2)])   # N = 9: the masked tail alone
def test_short_windows_take_the_tiled_schedules(engine, kid, N, d):
    """Shapes the marginal call sends to the one-launch short-window kernel: the joint calls answer from the tiled schedules;
    mean / diag(cov) agree with the marginal call to rounding."""
    B, M = 5, 33
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 5 + N)
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, cov, logml, info = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid)
    assert rc == 0
    rc, pm, pv, plm, _ = ctx.fit_predict_batch(X, y, Xs, theta, kid)
    np.testing.assert_allclose(mean, pm, rtol=0, atol=1e-9 * np.max(np.abs(pm)))
    np.testing.assert_allclose(np.diagonal(cov, axis1=1, axis2=2), pv, rtol=1e-8)
    for b in range(B):
        close(mean[b], cov[b], *oracle_joint(kid, theta[b], X[b], y[b], Xs[b]))


@pytest.mark.parametrize("N", [134, 301])
@pytest.mark.parametrize("M", [1, 17, 127, 128, 599])
def test_shapes_off_the_tile_boundaries(engine, N, M):
    """N not a multiple of 128, 16 or 4; M = 1, 17, 599; M + 1 crossing a 128-row tile (127, 128).  Exact symmetry."""
    d, kid, B = 2, 1, 2
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, N * M)
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, cov, _, info = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=False)
    assert rc == 0 and np.array_equal(cov, cov.transpose(0, 2, 1))
    for b in range(B):
        close(mean[b], cov[b], *oracle_joint(kid, theta[b], X[b], y[b], Xs[b], False))


def test_joint_calls_leave_the_resident_fit_alone(engine):
    """cgp_get_factor, cgp_get_alpha, cgp_predict after the single-fit joint calls: bitwise what they give without them."""
    N, d, M, kid = 200, 2, 40, 1
    X, y, Xs, theta, rng = problem(1, N, d, M, kid, 3)
    xi = rng.normal(size=(2, M))
    outs = []
    for between in (True, False):
        ctx = ctx_for(engine, 1, N, d, M)
        assert ctx.fit(X[0], y[0], kid, theta[0])[0] == 0
        if between:
            ctx.predict_cov(Xs[0])
            ctx.sample(Xs[0], xi)
            ctx.predict_cov(Xs[0][:3], include_noise=False)
        outs.append((ctx.factor(), ctx.alpha()) + ctx.predict(Xs[0]))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_jitter_ladder_is_per_fit_and_contracts_the_right_slab(engine):
    """test_gpu_parity.py::test_batch_jitter_retry_is_per_fit's input at N = 200 (the marginal call is tiled too): fit 1 needs
    the first rung; it is re-submitted as a call of one fit whose factor lands in slab 0.  Its mean / diag(cov) are bitwise
    cgp_fit_predict_batch's, its covariance meets the oracle's jittered refit at 1e-5 (the bar the existing test holds that
    near-singular fit to; fp64 against 80-bit arithmetic on this input: 5.4e-9), fits 0 and 2 are bitwise what they are without
    the bad neighbour."""
    rng = np.random.default_rng(21)
    N, d, M, B = 200, 1, 7, 3
    X = np.stack([np.sort(rng.normal(size=(N, d)), 0) for _ in range(B)])
    Xgood = X.copy()
    X[1, :, 0] = np.repeat(np.arange(N // 2, dtype=float), 2)         # duplicated inputs -> rank deficient K
    y, ygood = np.sin(X[:, :, 0]), np.sin(Xgood[:, :, 0])
    Xs = np.tile(np.linspace(-1, 1, M)[None, :, None], (B, 1, 1))
    th = np.array([[1.0, 1.0, 0.05], [1.0, 3.0, -1e-8 - 2e-7], [1.0, 1.0, 0.05]])   # window 1: slightly indefinite
    thgood = np.array([[1.0, 1.0, 0.05]] * 3)
    f1 = go.fit(0, th[1], X[1], y[1])
    assert f1.jitter > 0
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, cov, logml, info = ctx.fit_predict_cov_batch(X, y, Xs, th, 0, include_noise=False)
    assert rc == 0 and not info.any()
    rc, pm, pv, plm, pinfo = ctx.fit_predict_batch(X, y, Xs, th, 0, include_noise=False)
    assert rc == 0 and np.array_equal(mean, pm) and np.array_equal(np.diagonal(cov, axis1=1, axis2=2), pv)
    close(mean[1], cov[1], *sliding_window_joint(0, th[1], N, X[1], y[1], Xs[1], include_noise=False), tol=1e-5)
    for b in (0, 2):
        close(mean[b], cov[b], *sliding_window_joint(0, th[b], N, X[b], y[b], Xs[b], include_noise=False))
    rc, gm, gc, _, _ = ctx.fit_predict_cov_batch(Xgood, ygood, Xs, thgood, 0, include_noise=False)
    assert rc == 0
    for b in (0, 2):
        assert np.array_equal(gm[b], mean[b]) and np.array_equal(gc[b], cov[b])
    xi = rng.normal(size=(B, 3, M))
    rc, paths, _, info, sinfo = ctx.fit_sample_batch(X, y, Xs, th, 0, xi, include_noise=False, jitter_rel=1e-6)
    _, gpaths, _, _, _ = ctx.fit_sample_batch(Xgood, ygood, Xs, thgood, 0, xi, include_noise=False, jitter_rel=1e-6)
    assert rc in (0, 2) and not info.any() and sinfo[0] == 0 and sinfo[2] == 0   # (fit 1's 7 x 7 matrix is all but singular)
    assert np.array_equal(paths[[0, 2]], gpaths[[0, 2]])


def device_arrays(torch, X, y, Xs, theta):
    B = X.shape[0]
    th = np.zeros((B, 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, Xs.transpose(0, 2, 1), th)]


def test_device_form_failed_fit_is_nan_neighbours_are_right(engine):
    import torch
    B, N, d, M, kid, S = 3, 200, 2, 30, 1, 4
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 8)
    theta[1, -1] = -2.0 * theta[1, 0]   # Ky of fit 1 is negative definite: no ladder in the device form
    xi = rng.normal(size=(B, S, M))
    ctx = ctx_for(engine, B, N, d, M)
    dX, dy, dXs, dth = device_arrays(torch, X, y, Xs, theta)
    dxi = torch.from_numpy(xi).cuda()
    dm = torch.zeros((B, M), dtype=torch.float64, device="cuda")
    dc = torch.zeros((B, M, M), dtype=torch.float64, device="cuda")
    dp = torch.zeros((B, S, M), dtype=torch.float64, device="cuda")
    dl = torch.zeros(B, dtype=torch.float64, device="cuda")
    di = torch.zeros(B, dtype=torch.int32, device="cuda")
    ds = torch.zeros(B, dtype=torch.int32, device="cuda")
    args = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0)
    assert ctx.fit_predict_cov_batch_device(*args, True, dm.data_ptr(), dc.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
    assert ctx.fit_sample_batch_device(*args, True, S, dxi.data_ptr(), 1e-6, dp.data_ptr(), dl.data_ptr(), di.data_ptr(), ds.data_ptr()) == 0
    torch.cuda.synchronize()
    info, sinfo, mean, cov, paths = (t.cpu().numpy() for t in (di, ds, dm, dc, dp))
    assert info[1] > 0 and info[0] == 0 and info[2] == 0
    assert np.all(np.isnan(cov[1])) and np.all(np.isnan(paths[1])) and sinfo[1] > 0 and sinfo[0] == 0 and sinfo[2] == 0
    for b in (0, 2):
        omu, ocov = oracle_joint(kid, theta[b], X[b], y[b], Xs[b])
        close(mean[b], cov[b], omu, ocov)
        op = sample_paths(omu, ocov - go.noise_var(kid, theta[b]) * np.eye(M), go.noise_var(kid, theta[b]), 1e-6, xi[b])
        assert np.max(np.abs(paths[b] - op)) <= TOL * np.max(np.abs(op))


@pytest.mark.parametrize("kid,N,d,M", [(1, 300, 3, 45), (2, 200, 1, 100), (0, 170, 2, 16), (3, 256, 3, 64)])
def test_paths_factor_and_random_draws(engine, kid, N, d, M):
    """xi = unit vectors returns C: lower triangular, C C^T = the device's own matrix (cov + noise + jitter) to 1e-9 and the
    oracle's at the bar; random xi against sample_paths, S = 1 and 50."""
    X, y, Xs, theta, rng = problem(1, N, d, M, kid, 31 + N)
    ctx = ctx_for(engine, 1, N, d, M)
    _, mean, cov, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=False)
    omu, ocov = oracle_joint(kid, theta[0], X[0], y[0], Xs[0], False)
    for noise in (False, True):
        sn = noise_of(kid, theta[0]) if noise else 0.0
        rc, out, _, _, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, np.eye(M)[None], include_noise=noise, jitter_rel=1e-6)
        assert rc == 0 and sinfo[0] == 0
        C = (out[0] - mean[0][None, :]).T   # path s = mean + column s of C
        assert np.array_equal(np.triu(C, 1), np.zeros((M, M)))
        A, Ad = sample_matrix(ocov, sn, 1e-6), sample_matrix(cov[0], sn, 1e-6)
        assert np.max(np.abs(C @ C.T - Ad)) <= 1e-9 * np.max(np.diag(Ad))
        assert np.max(np.abs(C @ C.T - A)) <= TOL * np.max(np.diag(A))
        for S in (1, 50):
            xi = rng.normal(size=(1, S, M))
            rc, out, _, _, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=noise, jitter_rel=1e-6)
            dev = mean[0][None, :] + xi[0] @ C.T
            assert out.shape == (1, S, M) and np.max(np.abs(out[0] - dev)) <= 1e-12 * np.max(np.abs(dev))
            if noise:   # well conditioned: the factor itself is in parity
                op = sample_paths(omu, ocov, sn, 1e-6, xi[0])
                assert np.max(np.abs(out[0] - op)) <= TOL * np.max(np.abs(op))


def test_rank_deficient_request_is_reported_not_fatal(engine):
    """Fit 1 asks for each of twelve points three times: without jitter and noise its matrix is singular -- reported in sinfo with
    NaN paths; the other fits' paths are right; with jitter_rel = 1e-6 the same request succeeds.
    Why twelve points and not one point many times: on the copies of ONE point the matrix is c 1 1^T + (v - c) I, with v the
    fit's variance (the diagonal) and c the contraction's value of the same quantity (prior - |V|^2, summed in another order).
    It is positive definite exactly when v > c: one rounding difference decides for all copies of a point, however many.  The
    points are training inputs, where the contraction rounds at the prior's ulp in every step, so v - c has either sign per
    point; the request passes only if all twelve differences are positive."""
    B, N, d, M, S, kid = 3, 200, 2, 40, 4, 1
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 33)
    Xs = Xs + 2.0 * rng.normal(size=Xs.shape)   # spread out: the other fits' matrices are comfortably positive definite
    Xs[1, :12] = X[1, -12:]
    Xs[1, 12:24] = Xs[1, :12]
    Xs[1, 24:36] = Xs[1, :12]
    xi = rng.normal(size=(B, S, M))
    ctx = ctx_for(engine, B, N, d, M)
    rc, out, _, info, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=False, jitter_rel=0.0)
    assert rc == 2 and not info.any() and sinfo[0] == 0 and sinfo[2] == 0 and 13 <= sinfo[1] <= 36
    assert np.all(np.isnan(out[1]))
    for b in (0, 2):
        omu, ocov = oracle_joint(kid, theta[b], X[b], y[b], Xs[b], False)
        op = sample_paths(omu, ocov, 0.0, 0.0, xi[b])
        assert np.max(np.abs(out[b] - op)) <= TOL * np.max(np.abs(op))
    rc, out, _, _, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=False, jitter_rel=1e-6)
    assert rc == 0 and not sinfo.any() and np.all(np.isfinite(out))


@pytest.mark.parametrize("B,N", [(3, 300), (60, 1024)])
def test_host_device_and_graph_replay_agree_bitwise(engine, B, N):
    """The legacy stream, CGP_STREAM_CTX and a captured side stream (B = 60, N = 1024: the mid-size schedule with the extra rows
    on a worker stream, joined before the contraction)."""
    import torch
    d, M, S, kid = 3, 53, 7, 1
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 9 + B)
    xi = rng.normal(size=(B, S, M))
    ctx = ctx_for(engine, B, N, d, M, reserve_m=64)
    rc, mean, cov, logml, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid)
    rc2, paths, _, _, _ = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=True, jitter_rel=1e-8)
    assert rc == 0 and rc2 == 0
    dX, dy, dXs, dth = device_arrays(torch, X, y, Xs, theta)
    dxi = torch.from_numpy(xi).cuda()
    dm = torch.empty((B, M), dtype=torch.float64, device="cuda")
    dc = torch.empty((B, M, M), dtype=torch.float64, device="cuda")
    dp = torch.empty((B, S, M), dtype=torch.float64, device="cuda")
    dl = torch.empty(B, dtype=torch.float64, device="cuda")
    di = torch.empty(B, dtype=torch.int32, device="cuda")
    ds = torch.empty(B, dtype=torch.int32, device="cuda")
    args = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0)

    def clear():
        for t in (dm, dc, dp, dl):
            t.fill_(-1.0)
        di.fill_(-1)
        ds.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dc.cpu().numpy(), cov)
        assert np.array_equal(dp.cpu().numpy(), paths) and np.array_equal(dl.cpu().numpy(), logml)
        assert not di.cpu().numpy().any() and not ds.cpu().numpy().any()

    def enqueue(s):
        assert ctx.fit_predict_cov_batch_device(*args, True, dm.data_ptr(), dc.data_ptr(), dl.data_ptr(), di.data_ptr(), stream=s) == 0
        assert ctx.fit_sample_batch_device(*args, True, S, dxi.data_ptr(), 1e-8, dp.data_ptr(), dl.data_ptr(), di.data_ptr(),
                                           ds.data_ptr(), stream=s) == 0

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


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.zeros(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 8, 1, 4, 2)   # batch, N, d, M, kernel

    def cov(h=ctx.h, shape=shape, xs=p, mean=p, c=p):
        return lib.cgp_fit_predict_cov_batch(h, *shape, p, p, xs, p, 4, 1, mean, c, p, ip)

    def smp(h=ctx.h, shape=shape, S=1, xi=p, jit=1e-6, out=p):
        return lib.cgp_fit_sample_batch(h, *shape, p, p, p, p, 4, 0, S, xi, jit, out, p, ip, ip)

    def covd(h=ctx.h, shape=shape, c=a):
        return lib.cgp_fit_predict_cov_batch_device(h, *shape, a, a, a, a, None, 1, a, c, a, a, None)

    def smpd(h=ctx.h, shape=shape, S=1, out=a):
        return lib.cgp_fit_sample_batch_device(h, *shape, a, a, a, a, None, 0, S, a, 1e-6, out, a, a, None, None)

    assert cov() == ESTATE and smp() == ESTATE and covd() == ESTATE and smpd() == ESTATE        # no reservation
    assert lib.cgp_predict_cov(ctx.h, p, 4, 1, p, p) == ESTATE and lib.cgp_sample(ctx.h, p, 4, 1, p, 0, 1e-6, p, ip) == ESTATE
    # the order of the answers: no context and M = 0 before the missing reservation ...
    calls = (cov, smp, covd, smpd)
    assert all(f(h=None) == EINVAL and f(shape=(1, 9, 1, 0, 2)) == EINVAL for f in calls) and lib.cgp_joint_reserve(None, 1, 4) == EINVAL
    for mb, mm in ((0, 4), (3, 4), (1, 0), (1, 9)):
        assert lib.cgp_joint_reserve(ctx.h, mb, mm) == EINVAL
    assert lib.cgp_joint_reserve(ctx.h, 1, 4) == 0
    assert lib.cgp_predict_cov(ctx.h, p, 4, 1, p, p) == ESTATE                                   # reserved, but nothing fitted
    big_m, big_b = (1, 8, 1, 5, 2), (2, 8, 1, 4, 2)
    for s in (big_m, big_b):
        assert cov(shape=s) == ECAPACITY and smp(shape=s) == ECAPACITY and covd(shape=s) == ECAPACITY and smpd(shape=s) == ECAPACITY
    for s in ((2, 9, 1, 1, 2), (1, 9, 1, 5, 2)):                                                 # ... the capacity before the arrays
        assert cov(shape=s, c=None) == ECAPACITY and smp(shape=s, S=0) == ECAPACITY
        assert covd(shape=s, c=None) == ECAPACITY and smpd(shape=s, out=None) == ECAPACITY
    m0 = (1, 8, 1, 0, 2)
    assert cov(shape=m0) == EINVAL and smp(shape=m0) == EINVAL and covd(shape=m0) == EINVAL and smpd(shape=m0) == EINVAL
    assert cov(xs=None) == EINVAL and cov(mean=None) == EINVAL and cov(c=None) == EINVAL and covd(c=None) == EINVAL
    assert smp(S=0) == EINVAL and smp(xi=None) == EINVAL and smp(out=None) == EINVAL and smpd(S=0) == EINVAL and smpd(out=None) == EINVAL
    assert smp(jit=-1e-6) == EINVAL and smp(jit=float("nan")) == EINVAL
    assert lib.cgp_sample(ctx.h, p, 4, 0, p, 0, 1e-6, p, ip) == EINVAL and lib.cgp_predict_cov(ctx.h, p, 0, 1, p, p) == EINVAL
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_joint_reserve(f32.h, 1, 4) == EINVAL
    assert cov(h=f32.h) == EINVAL and smp(h=f32.h) == EINVAL and covd(h=f32.h) == EINVAL and smpd(h=f32.h) == EINVAL
    assert lib.cgp_predict_cov(f32.h, p, 4, 1, p, p) == EINVAL and lib.cgp_sample(f32.h, p, 4, 1, p, 0, 1e-6, p, ip) == EINVAL
    # both contexts are still usable
    X, y, Xs, theta, rng = problem(1, 8, 1, 4, 2, 1)
    for c, tol in ((ctx, 1e-6), (f32, 1e-3)):
        rc, mean, var, _, _ = c.fit_predict_batch(X, y, Xs, theta, 2)
        omu, ocov = oracle_joint(2, theta[0], X[0], y[0], Xs[0])
        assert rc == 0 and np.max(np.abs(mean[0] - omu)) <= tol * np.max(np.abs(omu))
    rc, mean, cv, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, 2)
    close(mean[0], cv[0], omu, ocov)
    assert ctx.joint_reserve(2, 8) == 0   # a second reservation replaces the first
    X, y, Xs, theta, rng = problem(2, 8, 1, 8, 2, 2)
    rc, mean, cv, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, 2)
    assert rc == 0
    close(mean[1], cv[1], *oracle_joint(2, theta[1], X[1], y[1], Xs[1]))


def test_optimised_fits_feed_the_stop_time_lookahead(engine):
    """cgp_optimize_batch -> cgp_fit_sample_batch -> cgp_predict_stop_batch on the reference's window: 599 ticks, 64 paths, every
    member against go.predict_stop on its own path."""
    M, S, kid = 599, 64, 2
    tw, sw = synth.reference_window(n=149, tick0=11, seed=4000)
    X, y = tw[None, :, None], sw[None]
    ctx = ctx_for(engine, 1, 149, 1, M)
    theta, logml, nev = ctx.optimize_batch(X, y, kid, np.ones(4), max_evals=200)
    Xs = X[:, -1:, :] + 1.0 + np.arange(M, dtype=np.float64)[None, :, None]
    xi = np.random.default_rng(64).normal(size=(1, S, M))
    rc, paths, lm, info, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=False, jitter_rel=1e-6)
    assert rc == 0 and info[0] == 0 and sinfo[0] == 0
    omu, ocov = oracle_joint(kid, theta[0], X[0], y[0], Xs[0], False)
    _, mean, cov, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=False)
    close(mean[0], cov[0], omu, ocov)
    p = paths[0]
    sd = np.sqrt(np.diag(ocov))
    assert np.max(np.abs(p.mean(0) - omu) / sd) < 1.0   # 64 draws: the ensemble mean within a few standard errors
    st = synth.filter_state(2000)
    P, Q, STM, Hv, pos = (np.stack([st[j]] * S) for j in range(5))
    fired, cmd, iout, xy = ctx.predict_stop_batch(p, np.zeros_like(p), P, Q, STM, Hv, pos, 50.0, 50.2)
    for s in range(S):
        ef, ec, ei, exy = go.predict_stop(p[s], np.zeros(M), P[s], Q[s], STM[s], go.unpack_H(Hv[s], True), pos[s], 50.0, 50.2)
        assert bool(fired[s]) == ef and iout[s] == ei
        assert cmd[s] == pytest.approx(ec, rel=1e-12) and xy[s] == pytest.approx(exy, rel=1e-6)
