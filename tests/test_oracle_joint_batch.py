"""The identity the batch path's joint forecast rests on, checked on the oracle alone: the posterior covariance at Xs is the Schur
complement of the augmented matrix [[Ky, K*], [K*^T, K**]], and the rows the augmented Cholesky factor holds below L are
V^T = (L^-1 K*)^T -- so cov = K** - V^T V needs nothing but the factor panel.  Also the closed-form two-sample fixture."""
import numpy as np
import pytest
import scipy.linalg as sla

from conftest import load_golden
from oracle import gp_oracle as go
from joint_oracle import sliding_window_joint, sample_paths
import matern_oracle as mo
import corenav_gp_amd.synth as synth


def case(kid, N, d, M, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if kid == 2:
        return t[:, None], y, t[-1] + 1.0 + np.arange(M, dtype=np.float64)[:, None], np.array([0.5, 30.0, 0.01, 0.002])
    X = np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)])
    Xs = X[rng.integers(0, N, size=M)] + 0.3 * rng.normal(size=(M, d))
    theta = np.array([0.02, 1.0, 1e-3]) if kid == 0 else np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
    return X, y, Xs, theta


@pytest.mark.parametrize("kid,N,d,M", [(0, 60, 2, 25), (1, 134, 6, 40), (2, 134, 1, 50), (3, 80, 3, 30), (4, 80, 3, 30)])
def test_posterior_covariance_is_the_schur_complement_of_the_augmented_matrix(kid, N, d, M):
    X, y, Xs, theta = case(kid, N, d, M, 10 * N + kid)
    mod, fit = (mo, mo.fit(kid, theta, X, y)) if kid >= 3 else (go, go.fit(kid, theta, X, y))
    assert fit.jitter == 0.0
    Ks, Kss = mod.kernel_K(kid, theta, X, Xs), mod.kernel_K(kid, theta, Xs)
    Ky = fit.L @ fit.L.T
    if kid >= 3:
        mean, cov = mo.predict_cov(fit, Xs, include_noise=False)
    else:
        mean, cov = sliding_window_joint(kid, theta, N, X, y, Xs, include_noise=False)
    assert np.min(np.diag(cov)) > 10 * go.GPY_VAR_FLOOR   # the clip is not what is compared
    sd = np.sqrt(np.diag(cov))
    schur = Kss - Ks.T @ np.linalg.solve(Ky, Ks)
    assert np.max(np.abs(schur - cov) / np.outer(sd, sd)) < 1e-8
    # the augmented factor: its extra rows are V^T, and what is left of K** below them is the covariance (+ the ridge that makes
    # the augmented matrix factorable at all when cov is numerically singular)
    ridge = 1e-6 * np.mean(np.diag(Kss))
    A = np.block([[Ky, Ks], [Ks.T, Kss + ridge * np.eye(M)]])
    La = np.linalg.cholesky(A)
    Vt = La[N:, :N]
    np.testing.assert_allclose(La[:N, :N], fit.L, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(Vt.T, sla.solve_triangular(fit.L, Ks, lower=True), rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(Kss - Vt @ Vt.T - cov) / np.outer(sd, sd)) < 1e-8
    L22 = La[N:, N:]
    assert np.max(np.abs(L22 @ L22.T - ridge * np.eye(M) - cov) / np.outer(sd, sd)) < 1e-7
    np.testing.assert_allclose(mean, Vt @ sla.solve_triangular(fit.L, y, lower=True), rtol=1e-8, atol=1e-10)


def test_batch_oracle_route_against_the_closed_form_of_two_samples():
    g = load_golden("closed_joint_n2_se")
    kid, theta, X, y, Xs = int(g["kernel_id"]), g["theta"], g["X"], g["y"], g["Xs"]
    f = go.fit(kid, theta, X.reshape(2, -1), y)
    Ks = go.kernel_K(kid, theta, f.X, Xs.reshape(len(Xs), -1))
    V = sla.solve_triangular(f.L, Ks, lower=True)
    cov = go.kernel_K(kid, theta, Xs.reshape(len(Xs), -1)) - V.T @ V
    np.testing.assert_allclose(Ks.T @ f.alpha, g["mean"], rtol=1e-11)
    np.testing.assert_allclose(cov, g["cov_latent"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(sample_paths(g["mean"], cov, float(g["noise"]), float(g["jitter_rel"]), g["xi"]), g["paths"], rtol=1e-9)
