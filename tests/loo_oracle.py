"""float64 oracle of leave-one-out cross-validation (cgp_loo*, cgp_window_loo*): GPy's inference_method.LOO, Rasmussen &
Williams eq. 5.10-5.12, on the quantities of oracle.gp_oracle.fit (kernel ids 0-2) or tests/matern_oracle.fit (ids 3, 4) --
the jitter ladder included, the jitter counted in loo_var:

    Ky = K + (sigma_n^2 + 1e-8 + jitter) I,  alpha = Ky^-1 y,  kd_i = [Ky^-1]_ii
    loo_var_i = 1 / kd_i      loo_mean_i = y_i - alpha_i / kd_i
    loo_lpd_i = -0.5 log(2 pi loo_var_i) - 0.5 (y_i - loo_mean_i)^2 / loo_var_i      lpd_sum = sum_i loo_lpd_i

loo_brute is the definition itself: N refits with one sample deleted, each predicting the deleted (noisy) sample."""
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo

LOG_2PI = float(np.log(2.0 * np.pi))
Loo = namedtuple("Loo", "mean var lpd lpd_sum logml jitter")


def fit(kid, theta, X, y):
    """The go.Fit of the window with Kyinv set, whichever oracle knows the kernel."""
    if kid in mo.KERNELS:
        f = mo.fit(kid, theta, X, y)
        Li = sla.solve_triangular(f.L, np.eye(len(f.y)), lower=True)
        f.Kyinv = Li.T @ Li
        return f
    return go.fit(kid, theta, X, y, want_inverse=True)


def lpd_of(y, mean, var):
    return -0.5 * np.log(2.0 * np.pi * var) - 0.5 * (y - mean) ** 2 / var


def loo(kid, theta, X, y):
    """Closed form.  Raises go.NotPositiveDefinite where the jitter ladder gives up."""
    f = fit(kid, theta, X, y)
    kd = np.diag(f.Kyinv).copy()
    var = 1.0 / kd
    mean = f.y - f.alpha / kd
    lpd = lpd_of(f.y, mean, var)
    return Loo(mean, var, lpd, float(np.sum(lpd)), f.logml, f.jitter)


def ky_of(kid, theta, X, jitter=0.0):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    theta = np.asarray(theta, dtype=np.float64)
    Ky = (mo.kernel_K if kid in mo.KERNELS else go.kernel_K)(kid, theta, X).copy()
    noise = mo.noise_var(theta) if kid in mo.KERNELS else go.noise_var(kid, theta)
    Ky[np.diag_indices(len(X))] += noise + go.GPY_DIAG_EPS + jitter
    return Ky


def loo_brute(kid, theta, X, y, jitter=0.0):
    """N refits on N - 1 samples at the diagonal the full fit ended with; sample i predicted with noise."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = len(y)
    Ky = ky_of(kid, theta, X, jitter)
    mean, var = np.zeros(N), np.zeros(N)
    for i in range(N):
        keep = np.arange(N) != i
        var[i] = Ky[i, i]
        if N > 1:
            c = sla.cho_factor(Ky[np.ix_(keep, keep)], lower=True)
            k = Ky[keep, i]
            mean[i] = k @ sla.cho_solve(c, y[keep])
            var[i] -= k @ sla.cho_solve(c, k)
    lpd = lpd_of(y, mean, var)
    return Loo(mean, var, lpd, float(np.sum(lpd)), None, jitter)


def check(got, want, y, bar=1e-6):
    """The project's fp64 bar on (loo_mean, loo_var, loo_lpd, lpd_sum) against a Loo; returns the four scaled errors."""
    gm, gv, gl, gs = got
    e = (np.max(np.abs(gm - want.mean)) / max(1.0, float(np.max(np.abs(y)))),
         np.max(np.abs(gv - want.var) / want.var),
         np.max(np.abs(gl - want.lpd) / np.maximum(1.0, np.abs(want.lpd))),
         abs(gs - want.lpd_sum) / max(1.0, float(np.sum(np.abs(want.lpd)))))
    assert all(np.isfinite(e)) and max(e) <= bar, e
    return e
