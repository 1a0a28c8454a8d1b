"""CPU: the multi-target oracle helper (tests/multi_oracle.py, one refit per column) against an independent restatement of what
the engine computes -- ONE Cholesky, Z = L^-1 Y by 128-column blocks with explicit block inverses, mean = V^T Z, logml[p] =
-1/2 |Z_p|^2 - sum log L_ii - N/2 log 2 pi -- and GPy's summed objective.  Bar 1e-10: two orderings of the same double-precision
sums (measured: <= 4e-13 for RBF x Brownian at N = 257, P = 5, M = 129), more than 100 x margin."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp_oracle as go
from multi_oracle import fit_predict_multi, errors
import corenav_gp_amd.synth as synth

TOL = 1e-10
TS = 128


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])


def problem(kid, N, P, M, seed):
    d = 1 if kid == 2 else 3
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + N, dtype=np.float64)
    Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1 + p), t) for p in range(P)])
    if d == 1:
        X, Xs = t[:, None], t[-1] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    else:
        X = np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)])
        Xs = X[rng.integers(max(0, N - 50), N, size=M)] + 0.3 * rng.normal(size=(M, d))
    return X, Y, Xs, theta_of(kid, d)


def restatement(kid, theta, X, Y, Xs, noise):
    """One factor; the forward solve the way the engine blocks it: Z(:, k) = (Y(:, k) - sum_{j<k} Z(:, j) L(k, j)^T) W_k^T."""
    N = len(X)
    Ky = go.kernel_K(kid, theta, X)
    Ky[np.diag_indices(N)] += go.noise_var(kid, theta) + go.GPY_DIAG_EPS
    L = np.linalg.cholesky(Ky)
    Z = np.zeros_like(Y)   # (P, N): row p is (L^-1 y_p)^T
    for k0 in range(0, N, TS):
        k1 = min(k0 + TS, N)
        W = sla.solve_triangular(L[k0:k1, k0:k1], np.eye(k1 - k0), lower=True)   # W_k = L(k,k)^-1
        Z[:, k0:k1] = (Y[:, k0:k1] - Z[:, :k0] @ L[k0:k1, :k0].T) @ W.T
    V = sla.solve_triangular(L, go.kernel_K(kid, theta, X, Xs), lower=True)
    mean = Z @ V
    var = np.clip(go.kernel_Kdiag(kid, theta, Xs) - np.sum(V * V, 0), 1e-15, np.inf)
    if noise:
        var = var + go.noise_var(kid, theta)
    sumlog = float(np.sum(np.log(np.diag(L))))
    logml = -0.5 * np.sum(Z * Z, axis=1) - sumlog - 0.5 * N * np.log(2.0 * np.pi)
    return mean, var, logml, Ky


@pytest.mark.parametrize("kid", [0, 1, 2])
@pytest.mark.parametrize("N", [128, 130, 257])
def test_helper_against_one_factor_restatement(kid, N):
    P, M = 5, 129
    X, Y, Xs, theta = problem(kid, N, P, M, 100 * kid + N)
    for noise in (True, False):
        omean, ovar, ologml = fit_predict_multi(kid, theta, X, Y, Xs, noise)
        assert omean.shape == (P, M) and ovar.shape == (M,) and ologml.shape == (P,)
        mean, var, logml, Ky = restatement(kid, theta, X, Y, Xs, noise)
        em, ev, el = errors(mean, var, logml, omean, ovar, ologml)
        print(f"kernel {kid} N {N} noise {noise}: mean {em:.3g} var {ev:.3g} logml {el:.3g}")
        assert em <= TOL and ev <= TOL and el <= TOL, (em, ev, el)
    # GPy's objective for Y (N, P): sum_p logml[p] = -P/2 log|Ky| - 1/2 tr(Y^T Ky^-1 Y) - N P / 2 log 2 pi
    _, logdet = np.linalg.slogdet(Ky)
    obj = -0.5 * P * logdet - 0.5 * np.trace(Y @ np.linalg.solve(Ky, Y.T)) - 0.5 * N * P * np.log(2.0 * np.pi)
    assert abs(np.sum(ologml) - obj) <= TOL * max(1.0, abs(obj))
