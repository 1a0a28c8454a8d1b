"""Oracle of the sparse (inducing-point) fits (cgp_fit_predict_sparse_batch): a numpy / scipy restatement of include/corenav_gp.h's
definition -- the collapsed variational bound of Titsias (2009), GPy's SparseGPRegression / VarDTC, in its B = I + A form -- on
oracle/gp_oracle.py's kernels (tests/matern_oracle.py's for the Matern ids).  It also reports what the comparisons are conditioned
on: whether K_uu needed the jitter ladder, cond(K_uu) and cond(B)."""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo
import multi_oracle

LOG_2PI = float(np.log(2.0 * np.pi))
DIAG_EPS = 1e-8                  # the dense path's diagonal: sigma2 = sigma_n^2 + 1e-8
MAX_COND_UU, MAX_COND_B = 1e6, 1e8   # the conditions on every compared input (test_oracle_sparse.py asserts them)
VAR_FLOOR = 1e-15


def _mod(kid):
    return mo if kid >= 3 else go


def _2d(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def ladder_jitters(kid, theta, Z):
    """The engine's jitter ladder on K_uu: mean(diag(K(Z, Z))) + sigma_n^2 + 1e-8, times 1e-6 10^k, k = 0 .. 4."""
    base = float(np.mean(_mod(kid).kernel_Kdiag(kid, theta, _2d(Z)))) + float(theta[-1]) + DIAG_EPS
    return [base * 1e-6 * 10.0 ** k for k in range(5)]


def _first_bad_pivot(A):
    """1-based index of the first non-positive pivot of the unpivoted Cholesky of A (0: none) and the factor."""
    L, info = sla.lapack.dpotrf(np.ascontiguousarray(A), lower=1)
    if info == 0:   # (an optimised dpotrf does not test its pivots for NaN: the first diagonal entry that is not a positive number)
        odd = np.flatnonzero(~(np.diag(L) > 0.0) | ~np.isfinite(np.diag(L)))
        info = int(odd[0]) + 1 if len(odd) else 0
    return (np.tril(L), 0) if info == 0 else (None, int(info))


def fit_predict_sparse(kid, theta, X, y, Z, Xs, noise=True, eps=1e-8, jitter=0.0):
    """X (N, d), y (N,), Z (m, d), Xs (M, d) or None -> a namespace with mean (M,), var (M,), bound, info (0, the failing pivot k of
    K_uu after the ladder, or m + k for B), ladder (steps K_uu needed), jitter (the last one tried), cond_uu, cond_b.  jitter > 0:
    that jitter and no ladder (the device form)."""
    o = _mod(kid)
    theta = np.asarray(theta, dtype=np.float64)
    X, Z = _2d(X), _2d(Z)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, m = len(X), len(Z)
    Xs = np.zeros((0, X.shape[1])) if Xs is None else _2d(Xs)
    M = len(Xs)
    sigma2 = float(theta[-1]) + DIAG_EPS
    Kzz = o.kernel_K(kid, theta, Z)
    out = SimpleNamespace(mean=np.full(M, np.nan), var=np.full(M, np.nan), bound=np.nan, info=0, ladder=0, jitter=float(jitter),
                          cond_uu=np.inf, cond_b=np.inf)
    Lu, bad = _first_bad_pivot(Kzz + (eps + jitter) * np.eye(m))
    if bad and jitter == 0.0:
        for jit in ladder_jitters(kid, theta, Z):
            out.ladder += 1
            out.jitter = jit
            Lu, bad = _first_bad_pivot(Kzz + (eps + jit) * np.eye(m))
            if not bad:
                break
    if bad:
        out.info = bad
        return out
    out.cond_uu = float(np.linalg.cond(Lu @ Lu.T))
    Kuf = o.kernel_K(kid, theta, Z, X)                       # (m, N)
    Phi, b = Kuf @ Kuf.T, Kuf @ y
    t = float(np.sum(o.kernel_Kdiag(kid, theta, X)))
    W = sla.solve_triangular(Lu, Phi, lower=True)
    A = sla.solve_triangular(Lu, W.T, lower=True) / sigma2
    A = 0.5 * (A + A.T)
    Bm = np.eye(m) + A
    LB, bad = _first_bad_pivot(Bm)
    if bad:
        out.info = m + bad
        return out
    out.cond_b = float(np.linalg.cond(Bm))
    c = sla.solve_triangular(LB, sla.solve_triangular(Lu, b, lower=True), lower=True) / sigma2
    out.bound = float(-0.5 * N * LOG_2PI - 0.5 * N * np.log(sigma2) - np.sum(np.log(np.diag(LB))) - y @ y / (2.0 * sigma2)
                      + 0.5 * c @ c - t / (2.0 * sigma2) + 0.5 * np.trace(A))
    if M:
        V1 = sla.solve_triangular(Lu, o.kernel_K(kid, theta, Z, Xs), lower=True)
        V2 = sla.solve_triangular(LB, V1, lower=True)
        out.mean = V2.T @ c
        var = o.kernel_Kdiag(kid, theta, Xs) - np.sum(V1 * V1, 0) + np.sum(V2 * V2, 0)
        var = np.clip(var, VAR_FLOOR, np.inf)
        out.var = var + float(theta[-1]) if noise else var
    return out


def conditions_hold(o):
    """The conditions on every input compared with the device: no ladder step, cond(K_uu) <= 1e6, cond(B) <= 1e8."""
    return o.info == 0 and o.ladder == 0 and o.cond_uu <= MAX_COND_UU and o.cond_b <= MAX_COND_B


def errors(mean, var, bound, o):
    """multi_oracle.errors' metric: the mean against the largest oracle mean, the variance relative, the bound against
    max(1, |bound|).  M = 0: the bound only."""
    if len(o.mean) == 0:
        return 0.0, 0.0, float(abs(bound - o.bound) / max(1.0, abs(o.bound)))
    em, ev, el = multi_oracle.errors(np.asarray(mean)[None], np.asarray(var), np.array([bound]), o.mean[None], o.var,
                                     np.array([o.bound]))
    return float(em), float(ev), float(el)
