"""Oracle of the sparse fits with P target columns (cgp_fit_predict_sparse_multi_batch), stated twice:
  per_column   the definition: the pinned tests/sparse_oracle.py once per column (any subset of the columns);
  one_factor   what the engine shares: K_uu, Phi, A and B factored once, C = L_B^-1 L_u^-1 K_uf Y^T / sigma2 for all columns at once,
               one variance.
tests/test_oracle_sparse_multi.py holds the two to each other at 1e-10 on every input the GPU tests compare."""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

import multi_oracle
import sparse_oracle as so


def per_column(kid, theta, X, Y, Z, Xs, noise=True, jitter=0.0, cols=None):
    """Y (P, N) -> mean (P, M), var (M,), bound (P,) with NaN rows for the columns not in `cols` (None: all), info, ladder, jitter,
    cond_uu, cond_b (functions of (X, Z, theta) alone: the first evaluated column's)."""
    Y = np.asarray(Y, dtype=np.float64)
    P = Y.shape[0]
    M = 0 if Xs is None else len(Xs)
    cols = range(P) if cols is None else sorted(set(cols))
    out = SimpleNamespace(mean=np.full((P, M), np.nan), var=np.full(M, np.nan), bound=np.full(P, np.nan), cols=list(cols))
    for n, p in enumerate(cols):
        o = so.fit_predict_sparse(kid, theta, X, Y[p], Z, Xs, noise, jitter=jitter)
        if n == 0:
            out.var, out.info, out.ladder, out.jitter, out.cond_uu, out.cond_b = o.var, o.info, o.ladder, o.jitter, o.cond_uu, o.cond_b
        else:
            assert np.array_equal(o.var, out.var, equal_nan=True) and o.info == out.info   # (the targets do not enter them)
        out.mean[p], out.bound[p] = o.mean, o.bound
    return out


def one_factor(kid, theta, X, Y, Z, Xs, noise=True, eps=1e-8, jitter=0.0):
    """The same model with everything that does not depend on the targets computed once (no ladder: jitter as given)."""
    o = so._mod(kid)
    theta = np.asarray(theta, dtype=np.float64)
    X, Z = so._2d(X), so._2d(Z)
    Y = np.asarray(Y, dtype=np.float64)
    P, N = Y.shape
    m = len(Z)
    Xs = np.zeros((0, X.shape[1])) if Xs is None else so._2d(Xs)
    sigma2 = float(theta[-1]) + so.DIAG_EPS
    Lu = np.linalg.cholesky(o.kernel_K(kid, theta, Z) + (eps + jitter) * np.eye(m))
    Kuf = o.kernel_K(kid, theta, Z, X)
    W = sla.solve_triangular(Lu, Kuf @ Kuf.T, lower=True)
    A = sla.solve_triangular(Lu, W.T, lower=True) / sigma2
    A = 0.5 * (A + A.T)
    LB = np.linalg.cholesky(np.eye(m) + A)
    C = sla.solve_triangular(LB, sla.solve_triangular(Lu, Kuf @ Y.T, lower=True), lower=True) / sigma2   # (m, P)
    t = float(np.sum(o.kernel_Kdiag(kid, theta, X)))
    shared = -0.5 * N * so.LOG_2PI - 0.5 * N * np.log(sigma2) - np.sum(np.log(np.diag(LB))) - t / (2.0 * sigma2) + 0.5 * np.trace(A)
    out = SimpleNamespace(shared=float(shared), C=C, mean=np.zeros((P, 0)), var=np.zeros(0), cols=list(range(P)))
    out.bound = shared - np.sum(Y * Y, axis=1) / (2.0 * sigma2) + 0.5 * np.sum(C * C, axis=0)
    if len(Xs):
        V1 = sla.solve_triangular(Lu, o.kernel_K(kid, theta, Z, Xs), lower=True)
        V2 = sla.solve_triangular(LB, V1, lower=True)
        out.mean = (V2.T @ C).T
        var = np.clip(o.kernel_Kdiag(kid, theta, Xs) - np.sum(V1 * V1, 0) + np.sum(V2 * V2, 0), so.VAR_FLOOR, np.inf)
        out.var = var + float(theta[-1]) if noise else var
    return out


def errors(mean, var, bound, o):
    """multi_oracle.errors' metric over the oracle's evaluated columns; M = 0: the bounds only."""
    c = o.cols
    mean, bound = np.asarray(mean), np.asarray(bound)
    el = float(np.max(np.abs(bound[c] - o.bound[c]) / np.maximum(1.0, np.abs(o.bound[c]))))
    if o.mean.shape[1] == 0:
        return 0.0, 0.0, el
    em, ev, el = multi_oracle.errors(mean[c], np.asarray(var), bound[c], o.mean[c], o.var, o.bound[c])
    return float(em), float(ev), float(el)
