"""Oracle of the multi-target objective (cgp_multi_nll_grad_batch, cgp_optimize_multi_batch): GPy.models.GPRegression(X, Y, kernel)
with Y (N, P) maximises sum_p logml[p] over ONE theta.  The columns are independent given theta, so the oracle is the sum of the
single-column restatements (go.nll_and_grad / matern_oracle.nll_and_grad), nothing shared; a second, one-factor restatement
1/2 (A A^T - P Ky^-1) pins that the sum is what GPy's ExactGaussianInference computes with P columns."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo


def _o(kid):
    return mo if kid >= 3 else go


def n_theta(kid, d):
    return _o(kid).n_theta(kid, d)


def nll_and_grad_multi(kid, theta, X, Y):
    """X (N, d), Y (P, N) -> (-sum_p logml[p], its gradient in natural parameters, logml (P,)): one oracle evaluation per column
    (GPy's jitter ladder included; the matrix is the same for every column, so is the jitter)."""
    o = _o(kid)
    nll, grad, lml = 0.0, 0.0, []
    for y in np.asarray(Y, dtype=np.float64):
        f, g = o.nll_and_grad(kid, theta, X, y)
        nll, grad = nll + f, grad + g
        lml.append(-f)
    return nll, grad, np.array(lml)


def nll_and_grad_one_factor(kid, theta, X, Y):
    """The same objective from one factorisation: Z = L^-1 Y, A = Ky^-1 Y, dL/dK = 1/2 (A A^T - P Ky^-1)."""
    o = _o(kid)
    theta = np.asarray(theta, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    Y = np.asarray(Y, dtype=np.float64)
    P, N = Y.shape
    Ky = o.kernel_K(kid, theta, X)
    Ky[np.diag_indices(N)] += float(theta[-1]) + go.GPY_DIAG_EPS
    L, _, _ = go.jitchol(Ky)
    Z = sla.solve_triangular(L, Y.T, lower=True)
    A = sla.solve_triangular(L, Z, lower=True, trans="T")
    Li = sla.solve_triangular(L, np.eye(N), lower=True)
    W = A @ A.T - P * (Li.T @ Li)
    nll = P * float(np.sum(np.log(np.diag(L)))) + 0.5 * float(np.sum(Z * Z)) + 0.5 * N * P * np.log(2.0 * np.pi)
    return nll, np.array([-0.5 * float(np.sum(W * dK)) for dK in o.dK_dtheta(kid, theta, X)])


def optimize_multi(kid, X, Y, theta0=None, max_evals=1000):
    """m.optimize() of the multi-column model, go.optimize's recipe on the summed objective: scipy L-BFGS-B without bounds over
    the Logexp-transformed parameters from all-ones.  A trial point that does not factor, or whose value or gradient is not
    finite, is infeasible.  Returns (theta, sum_p logml, evaluations, warnflag)."""
    import scipy.optimize as so
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    nth = n_theta(kid, X.shape[1])
    th0 = np.ones(nth) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    count = [0]

    def fg(x):
        count[0] += 1
        th = go.logexp(x)
        try:
            nll, g, _ = nll_and_grad_multi(kid, th, X, Y)
        except np.linalg.LinAlgError:
            return 1e300, np.zeros_like(x)
        if not (np.isfinite(nll) and np.all(np.isfinite(g))):
            return 1e300, np.zeros_like(x)
        return nll, g * -np.expm1(-th)        # dtheta/dx = 1 - exp(-theta)

    x, fval, dct = so.fmin_l_bfgs_b(fg, go.logexp_inv(th0), maxfun=max_evals)
    return go.logexp(x), -fval, count[0], dct["warnflag"]
