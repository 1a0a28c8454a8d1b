"""float64 oracle of the Matern 3/2 and 5/2 ARD kernels (CGP_KERNEL_MATERN32_ARD = 3, CGP_KERNEL_MATERN52_ARD = 4).
oracle/gp_oracle.py knows the three squared-exponential based kernels and is frozen, so the reference values of the Matern pair
come from this test-support module: numpy / scipy only, the textbook formulas, pinned independently by the fixtures
tests/golden/gen_matern_golden.py writes (scikit-learn, closed forms, a 50-digit mpmath factorisation) and checked against them by
tests/test_oracle_matern.py.  The inference steps (noise + 1e-8 on the diagonal, the jitter ladder, the variance floor) are the
ones oracle/gp_oracle.py documents; they do not depend on the kernel and are imported from there.

theta = [sigma_f^2, ell_1 .. ell_d, sigma_n^2] (natural parameters), r^2 = sum_q ((x_q - x'_q) / ell_q)^2
    MATERN32: k = sigma_f^2 (1 + sqrt(3) r) exp(-sqrt(3) r)
    MATERN52: k = sigma_f^2 (1 + sqrt(5) r + 5/3 r^2) exp(-sqrt(5) r)"""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go

KERNEL_MATERN32_ARD = 3
KERNEL_MATERN52_ARD = 4
KERNELS = (KERNEL_MATERN32_ARD, KERNEL_MATERN52_ARD)
LOG_2PI = float(np.log(2.0 * np.pi))


def n_theta(kernel_id, d):
    assert kernel_id in KERNELS
    return d + 2


def noise_var(theta):
    return float(theta[-1])


def _r2(theta, X, X2):
    """Scaled squared distances from coordinate DIFFERENCES (no inner-product expansion: exact zeros at coincident points)."""
    ell = np.asarray(theta[1:-1], dtype=np.float64)
    D = (X[:, None, :] - X2[None, :, :]) / ell[None, None, :]
    return np.sum(D * D, axis=2)


def radial(kernel_id, r2):
    """(k / sigma_f^2, dk/dr^2 / sigma_f^2) as functions of r^2; both are finite at r = 0 (no quotient by r)."""
    r2 = np.maximum(np.asarray(r2, dtype=np.float64), 0.0)
    if kernel_id == KERNEL_MATERN32_ARD:
        s = np.sqrt(3.0 * r2)
        e = np.exp(-s)
        return (1.0 + s) * e, -1.5 * e
    assert kernel_id == KERNEL_MATERN52_ARD
    s = np.sqrt(5.0 * r2)
    e = np.exp(-s)
    return (1.0 + s + (5.0 / 3.0) * r2) * e, -(5.0 / 6.0) * (1.0 + s) * e


def _as2d(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def kernel_K(kernel_id, theta, X, X2=None):
    theta = np.asarray(theta, dtype=np.float64)
    X = _as2d(X)
    X2 = X if X2 is None else _as2d(X2)
    return theta[0] * radial(kernel_id, _r2(theta, X, X2))[0]


def kernel_Kdiag(kernel_id, theta, X):
    return np.full(len(_as2d(X)), float(theta[0]))


def fit(kernel_id, theta, X, y):
    """Ky = K + (sigma_n^2 + 1e-8) I; L = jitchol(Ky) (go.jitchol: the GPy ladder); alpha; logML.  Returns a go.Fit."""
    theta = np.asarray(theta, dtype=np.float64)
    X = _as2d(X)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = len(y)
    Ky = kernel_K(kernel_id, theta, X)
    Ky[np.diag_indices(N)] += noise_var(theta) + go.GPY_DIAG_EPS
    L, jitter, _ = go.jitchol(Ky)
    z = sla.solve_triangular(L, y, lower=True)
    alpha = sla.solve_triangular(L, z, lower=True, trans="T")
    f = go.Fit()
    f.kernel_id, f.theta, f.X, f.y = kernel_id, theta, X, y
    f.L, f.alpha, f.z, f.jitter = L, alpha, z, jitter
    f.logml = 0.5 * (-N * LOG_2PI - 2.0 * float(np.sum(np.log(np.diag(L)))) - float(y @ alpha))
    f.Kyinv = None
    return f


def predict(f, Xs, include_noise=True):
    """mean, variance (clipped at 1e-15, + sigma_n^2 with include_noise) at Xs."""
    mean, cov = predict_cov(f, Xs, include_noise)
    return mean, np.diag(cov).copy()


def predict_cov(f, Xs, include_noise=True):
    """mean (M,), full posterior covariance (M, M): K** - V^T V, diagonal clipped at 1e-15, noise on the diagonal only."""
    Xs = _as2d(Xs)
    Ks = kernel_K(f.kernel_id, f.theta, f.X, Xs)
    V = sla.solve_triangular(f.L, Ks, lower=True)
    cov = kernel_K(f.kernel_id, f.theta, Xs) - V.T @ V
    cov = 0.5 * (cov + cov.T)
    i = np.arange(len(Xs))
    cov[i, i] = np.clip(cov[i, i], go.GPY_VAR_FLOOR, np.inf) + (noise_var(f.theta) if include_noise else 0.0)
    return Ks.T @ f.alpha, cov


def dK_dtheta(kernel_id, theta, X):
    """List of dK/dtheta_p (N x N each), natural parameters, noise last: dk/dell_q = dk/dr^2 (-2 d_q^2 / ell_q^3)."""
    theta = np.asarray(theta, dtype=np.float64)
    X = _as2d(X)
    N, d = X.shape
    k, dk = radial(kernel_id, _r2(theta, X, X))
    out = [k]
    for q in range(d):
        dq = X[:, None, q] - X[None, :, q]
        out.append(theta[0] * dk * (-2.0 * dq * dq / theta[1 + q] ** 3))
    out.append(np.eye(N))
    return out


def nll_and_grad(kernel_id, theta, X, y):
    """-logML and its gradient in natural parameters: dL/dK = 0.5 (alpha alpha^T - Ky^-1)."""
    f = fit(kernel_id, theta, X, y)
    Li = sla.solve_triangular(f.L, np.eye(len(f.y)), lower=True)
    W = np.outer(f.alpha, f.alpha) - Li.T @ Li
    return -f.logml, np.array([-0.5 * float(np.sum(W * dK)) for dK in dK_dtheta(kernel_id, theta, f.X)])


def optimize(kernel_id, X, y, theta0=None, max_evals=1000):
    """m.optimize() on this objective, go.optimize's recipe: scipy L-BFGS-B without bounds over the Logexp-transformed
    parameters from all-ones (GPy's defaults).  Returns (theta, logml, evaluations)."""
    import scipy.optimize as so
    X = _as2d(X)
    nth = n_theta(kernel_id, X.shape[1])
    th0 = np.ones(nth) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    count = [0]

    def fg(x):
        count[0] += 1
        th = go.logexp(x)
        try:
            nll, g = nll_and_grad(kernel_id, th, X, y)
        except np.linalg.LinAlgError:
            return 1e300, np.zeros_like(x)
        return nll, g * -np.expm1(-th)        # dtheta/dx = 1 - exp(-theta)

    x, fval, _ = so.fmin_l_bfgs_b(fg, go.logexp_inv(th0), maxfun=max_evals)
    return go.logexp(x), -fval, count[0]


def sliding_window_stream(kernel_id, theta, N, xs, ys, include_noise=True, record_at=()):
    """go.sliding_window_stream's contract for the Matern kernels: before a sample enters, predict it from the current window;
    then the oldest sample leaves if the window is full, the new one enters and the window is REFIT from scratch.  Returns
    (pred_mean, pred_var, logml) per tick; with record_at, also {tick: (X, y) of the window after that tick}."""
    xs = _as2d(xs)
    ys = np.asarray(ys, dtype=np.float64)
    T = len(ys)
    pm, pv, lm = np.zeros(T), np.zeros(T), np.zeros(T)
    Xw, yw = np.zeros((0, xs.shape[1])), np.zeros(0)
    rec = {}
    for t in range(T):
        if len(yw) >= N:
            Xw, yw = Xw[1:], yw[1:]
        if len(yw) == 0:
            pm[t], pv[t] = 0.0, theta[0] + (noise_var(theta) if include_noise else 0.0)
        else:
            mu, var = predict(fit(kernel_id, theta, Xw, yw), xs[t:t + 1], include_noise)
            pm[t], pv[t] = mu[0], var[0]
        Xw, yw = np.vstack([Xw, xs[t:t + 1]]), np.append(yw, ys[t])
        lm[t] = fit(kernel_id, theta, Xw, yw).logml
        if t in record_at:
            rec[t] = (Xw.copy(), yw.copy())
    return (pm, pv, lm, rec) if record_at else (pm, pv, lm)
