"""float64 oracle of the leave-one-out objective (cgp_loo_nll_grad*, cgp_optimize_loo_batch): nlpd = -lpd_sum of
tests/loo_oracle.py and its gradient with respect to the natural parameters, in closed form on loo_oracle.fit and the oracles'
dK_dtheta (Rasmussen & Williams 5.4.2):

    c_i = 1/2 (1 / kd_i + alpha_i^2 / kd_i^2)      b_i = alpha_i / kd_i      beta = Ky^-1 b
    d lpd_sum / dK = -Ky^-1 diag(c) Ky^-1 + 1/2 (beta alpha^T + alpha beta^T)

The noise sees dK / dsigma_n^2 = I; the jitter the ladder ended with is a constant of the evaluation.  central_difference is the
independent check: it differentiates loo_oracle.loo (or loo_brute) itself."""
import numpy as np

from oracle import gp_oracle as go
import matern_oracle as mo
import loo_oracle as lo


def _o(kid):
    return mo if kid in mo.KERNELS else go


def n_theta(kid, d):
    return _o(kid).n_theta(kid, d)


def _x2(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def dlpd_dK(f):
    """d lpd_sum / dK of a loo_oracle.fit record (symmetric N x N)."""
    Ki = f.Kyinv
    kd = np.diag(Ki)
    c = 0.5 * (1.0 / kd + f.alpha ** 2 / kd ** 2)
    beta = Ki @ (f.alpha / kd)
    return -(Ki * c[None, :]) @ Ki + 0.5 * (np.outer(beta, f.alpha) + np.outer(f.alpha, beta))


def nlpd_and_grad(kid, theta, X, y):
    """(nlpd, d nlpd / d theta, logml, jitter).  Raises go.NotPositiveDefinite where the jitter ladder gives up."""
    X = _x2(X)
    theta = np.asarray(theta, dtype=np.float64)
    f = lo.fit(kid, theta, X, y)
    kd = np.diag(f.Kyinv)
    lpd = lo.lpd_of(f.y, f.y - f.alpha / kd, 1.0 / kd)
    G = dlpd_dK(f)
    g = np.array([-float(np.sum(G * dK)) for dK in _o(kid).dK_dtheta(kid, theta, X)])
    return -float(np.sum(lpd)), g, f.logml, f.jitter


def central_difference(kid, theta, X, y, rel=1e-5, value=None):
    """Central differences of nlpd in every natural parameter, step rel * theta_i; value(theta) -> lpd_sum defaults to
    loo_oracle.loo's."""
    X = _x2(X)
    theta = np.asarray(theta, dtype=np.float64)
    if value is None:
        value = lambda th: lo.loo(kid, th, X, y).lpd_sum
    g = np.zeros(len(theta))
    for i in range(len(theta)):
        h = rel * abs(theta[i])
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        g[i] = -(value(tp) - value(tm)) / (2.0 * h)
    return g


def optimize_loo(kid, X, y, theta0=None, max_evals=1000):
    """multi_opt_oracle.optimize_multi's recipe on nlpd: scipy L-BFGS-B without bounds over the Logexp-transformed parameters from
    all-ones.  A trial point that does not factor, or whose value or gradient is not finite, is infeasible.  Returns (theta,
    lpd_sum, evaluations, warnflag)."""
    import scipy.optimize as so
    X = _x2(X)
    nth = n_theta(kid, X.shape[1])
    th0 = np.ones(nth) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    count = [0]

    def fg(x):
        count[0] += 1
        th = go.logexp(x)
        try:
            f, g, _, _ = nlpd_and_grad(kid, th, X, y)
        except np.linalg.LinAlgError:
            return 1e300, np.zeros_like(x)
        if not (np.isfinite(f) and np.all(np.isfinite(g))):
            return 1e300, np.zeros_like(x)
        return f, g * -np.expm1(-th)        # dtheta/dx = 1 - exp(-theta)

    x, fval, dct = so.fmin_l_bfgs_b(fg, go.logexp_inv(th0), maxfun=max_evals)
    return go.logexp(x), -fval, count[0], dct["warnflag"]
