"""Oracle of the explicit-basis (trend) calls (cgp_fit_predict_trend_batch, cgp_window_predict_trend): a numpy restatement of
include/corenav_gp.h's formulas (Rasmussen & Williams 2.7, eqs. 2.41, 2.42, 2.45 with a vague prior on beta) on oracle/gp_oracle.py's
kernels and Cholesky (tests/matern_oracle.py's for the Matern ids).  It also reports what the comparisons are conditioned on:
cond(A), the jitter the factor needed and the margin by which every pivot of A passes the rank rule."""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo

RANK_TOL = 1e-10          # include/corenav_gp.h, the rank rule
LOG_2PI = float(np.log(2.0 * np.pi))
MAX_COND, MIN_MARGIN = 1e6, 1e3   # the conditions on every compared input (test_oracle_trend.py asserts them)


def basis(x0, c, s, q):
    """[1, u, u^2][:q] with u = (x0 - c) / s -> (q, len(x0)): the basis used throughout the tests."""
    u = (np.asarray(x0, dtype=np.float64) - c) / s
    return np.stack([np.ones_like(u), u, u * u][:q])


def pivots(A):
    """The unpivoted Cholesky of A in index order under the rank rule -> (L_A or None, tinfo, margin): tinfo the 1-based pivot
    that is not > RANK_TOL * A[r][r] (0: none), margin the smallest pivot / (RANK_TOL * A[r][r]) met."""
    A = np.array(A, dtype=np.float64)
    q = len(A)
    d0 = np.diag(A).copy()
    L = np.zeros((q, q))
    margin = np.inf
    for r in range(q):
        piv = A[r, r]
        if not piv > RANK_TOL * d0[r]:
            return None, r + 1, 0.0
        margin = min(margin, piv / (RANK_TOL * d0[r]))
        L[r, r] = np.sqrt(piv)
        L[r + 1:, r] = A[r + 1:, r] / L[r, r]
        A[r + 1:, r + 1:] -= np.outer(L[r + 1:, r], L[r + 1:, r])
    return L, 0, margin


def fit_predict_trend(kid, theta, X, Y, H, Xs, Hs, noise=True):
    """X (N, d), Y (P, N), H (q, N), Xs (M, d), Hs (q, M) -> a namespace with mean (P, M), var (M,), base (M,) (the fit's own
    variance), beta (P, q), logml (P,), tinfo, cond (of A), jitter (of the factor), margin (of the rank rule).  A failed rank rule
    gives NaN outputs."""
    o = mo if kid >= 3 else go
    X = np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    Xs = np.asarray(Xs, dtype=np.float64)
    Xs = Xs[:, None] if Xs.ndim == 1 else Xs
    Y, H, Hs = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (Y, H, Hs))
    P, N = Y.shape
    q, M = Hs.shape
    f = o.fit(kid, theta, X, Y[0])
    L = f.L
    base = o.predict(f, Xs, noise)[1]
    Z = sla.solve_triangular(L, Y.T, lower=True)
    G = sla.solve_triangular(L, H.T, lower=True)
    V = sla.solve_triangular(L, o.kernel_K(kid, theta, X, Xs), lower=True)
    A, B = G.T @ G, G.T @ Z
    LA, tinfo, margin = pivots(A)
    out = SimpleNamespace(base=base, tinfo=tinfo, jitter=f.jitter, margin=margin,
                          cond=float(np.linalg.cond(A)) if np.all(np.isfinite(A)) else np.inf)
    if tinfo:
        nan = np.nan
        out.mean, out.var, out.beta, out.logml = np.full((P, M), nan), np.full(M, nan), np.full((P, q), nan), np.full(P, nan)
        return out
    W = sla.solve_triangular(LA, B, lower=True)                # L_A^-1 B
    beta = sla.solve_triangular(LA, W, lower=True, trans="T")  # (q, P)
    R = Hs - G.T @ V
    U = sla.solve_triangular(LA, R, lower=True)
    out.mean = Z.T @ V + beta.T @ R
    out.var = base + np.sum(U * U, 0)
    out.beta = beta.T
    out.logml = (-0.5 * np.sum(Z * Z, 0) + 0.5 * np.sum(W * W, 0) - np.sum(np.log(np.diag(L))) - np.sum(np.log(np.diag(LA)))
                 - 0.5 * (N - q) * LOG_2PI)
    return out


def conditions_hold(o):
    """The conditions on every compared input: no jitter, cond(A) <= 1e6, every pivot passes the rank rule by >= 1e3."""
    return o.tinfo == 0 and o.jitter == 0.0 and o.cond <= MAX_COND and o.margin >= MIN_MARGIN


def errors(mean, var, beta, logml, o):
    """multi_oracle.errors' metric extended to beta: a column's beta against that column's largest |beta|."""
    em = np.max(np.max(np.abs(mean - o.mean), axis=1) / np.maximum(np.max(np.abs(o.mean), axis=1), 1e-12))
    ev = np.max(np.abs(var - o.var) / o.var)
    eb = np.max(np.max(np.abs(beta - o.beta), axis=1) / np.maximum(np.max(np.abs(o.beta), axis=1), 1e-12))
    el = np.max(np.abs(logml - o.logml) / np.maximum(1.0, np.abs(o.logml)))
    return em, ev, eb, el
