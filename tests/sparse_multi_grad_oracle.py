"""Oracle of the sparse fits' objective with P target columns (cgp_sparse_multi_nll_grad_batch, cgp_optimize_sparse_multi_batch):
nll = -sum_p bound[p] on one (X, Z, theta) and its gradient in theta (natural parameters, cgp_nll_grad's order) and in the inducing
inputs Z, stated twice:
  per_column   the definition: the pinned tests/sparse_grad_oracle.py once per column, summed in column order;
  one_factor   what the engine shares: everything that does not depend on the targets once, with C = [c_1 ... c_P] (m x P):
                   Chat = L_B^-T C      M = L_u^-T Chat      Q = P (I - B^-1) - Chat Chat^T
                   T = L_u^-T Q L_u^-1 / (2 sigma2)      G_uu = 1/2 L_u^-T (Q - P A) L_u^-1      R = 2 T K_uf + M Y / sigma2
tests/test_oracle_sparse_multi_grad.py holds the two to each other at 1e-12 on every input the GPU tests compare.  Also the host
form's ladder and scipy's L-BFGS-B over [Logexp^-1(theta) | Z] in the manner of sparse_grad_oracle.optimize_sparse."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import sparse_oracle as so
import sparse_grad_oracle as sg


def per_column(kid, theta, X, Y, Z, jitter=0.0):
    """Y (P, N) -> (nll, grad (nth,), gradZ (m, d), logml (P,), info): sparse_grad_oracle.nll_grad per column, summed left to right."""
    Y = np.asarray(Y, dtype=np.float64)
    outs = [sg.nll_grad(kid, theta, X, y, Z, jitter=jitter) for y in Y]
    nll, g, gz, info = outs[0]
    logml = [-nll]
    for n, gp, gzp, _ in outs[1:]:
        nll, g, gz = nll + n, g + gp, gz + gzp
        logml.append(-n)
    return nll, g, gz, np.array(logml), info


def one_factor(kid, theta, X, Y, Z, jitter=0.0, eps=1e-8):
    """The same objective with one K_uu, one Phi, one pair of factors.  -> (nll, grad, gradZ, logml (P,), info); no ladder."""
    theta = np.asarray(theta, dtype=np.float64)
    X, Z = so._2d(X), so._2d(Z)
    Y = np.asarray(Y, dtype=np.float64)
    P, N = Y.shape
    m, d = Z.shape
    nth = sg.n_theta(kid, d)
    sigma2 = float(theta[-1]) + so.DIAG_EPS
    nan = (np.nan, np.full(nth, np.nan), np.full((m, d), np.nan), np.full(P, np.nan))
    Kuu, dKuu, dKuu_z = sg.kernel_parts(kid, theta, Z, Z, same=True)
    Lu, bad = so._first_bad_pivot(Kuu + (eps + jitter) * np.eye(m))
    if bad:
        return nan + (bad,)
    Kuf, dKuf, dKuf_z = sg.kernel_parts(kid, theta, Z, X)
    t = float(np.sum(so._mod(kid).kernel_Kdiag(kid, theta, X)))
    Li = sla.solve_triangular(Lu, np.eye(m), lower=True)
    A = Li @ (Kuf @ Kuf.T) @ Li.T / sigma2
    A = 0.5 * (A + A.T)
    LB, bad = so._first_bad_pivot(np.eye(m) + A)
    if bad:
        return nan + (m + bad,)
    # the columns' vectors one by one, in sparse_grad_oracle.nll_grad's own expressions: at P = 1 this IS that function
    total = lambda v: v[0] + sum(v[1:])
    LBi = sla.solve_triangular(LB, np.eye(m), lower=True)
    Binv = LBi.T @ LBi
    cs = [sla.solve_triangular(LB, Li @ (Kuf @ y), lower=True) / sigma2 for y in Y]
    logml = np.array([float(-0.5 * N * so.LOG_2PI - 0.5 * N * np.log(sigma2) - np.sum(np.log(np.diag(LB))) - y @ y / (2.0 * sigma2)
                            + 0.5 * c @ c - t / (2.0 * sigma2) + 0.5 * np.trace(A)) for y, c in zip(Y, cs)])
    chats = [LBi.T @ c for c in cs]
    mus = [Li.T @ ch for ch in chats]
    Q = P * (np.eye(m) - Binv) - total([np.outer(ch, ch) for ch in chats])
    T = Li.T @ Q @ Li / (2.0 * sigma2)
    Guu = 0.5 * Li.T @ (Q - P * A) @ Li
    R = 2.0 * T @ Kuf + total([np.outer(mu, y) for mu, y in zip(mus, Y)]) / sigma2
    dF = np.zeros(nth)
    for j, (duu, duf, dd) in enumerate(zip(dKuu, dKuf, sg.diag_parts(kid, theta, X))):
        dF[j] = np.sum(Guu * duu) + np.sum(R * duf) - P * np.sum(dd) / (2.0 * sigma2)
    dF[nth - 1] = (-N * P + (total([y @ y for y in Y]) + P * t) / sigma2 - P * np.trace(A) + P * m - P * np.trace(Binv)
                   - total([c @ c for c in cs]) - total([ch @ ch for ch in chats])) / (2.0 * sigma2)
    off = Guu - np.diag(np.diag(Guu))
    dZ = (np.einsum("ri,riq->rq", R, dKuf_z) + 2.0 * np.einsum("rs,rsq->rq", off, dKuu_z)
          + np.diag(Guu)[:, None] * dKuu_z[np.arange(m), np.arange(m), :])
    return -float(total(list(logml))), -dF, -dZ, logml, 0


def nll_grad_ladder(kid, theta, X, Y, Z):
    """The host form: the evaluation at the first jitter of sparse_oracle's ladder at which K_uu factors (0 first).
    -> (nll, grad, gradZ, logml, info, steps, jitter)."""
    out = one_factor(kid, theta, X, Y, Z)
    if out[4] == 0 or out[4] > len(so._2d(Z)):
        return out + (0, 0.0)
    for k, jit in enumerate(so.ladder_jitters(kid, theta, Z)):
        out = one_factor(kid, theta, X, Y, Z, jitter=jit)
        if out[4] == 0:
            break
    return out + (k + 1, jit)


def optimize_sparse_multi(kid, X, Y, Z0, theta0, optimize_z, max_evals=1000, factr=1e7):
    """SparseGPRegression(X, Y, Z=Z).optimize() with Y (P, N): sparse_grad_oracle.optimize_sparse on the summed objective.
    -> (theta, Z, summed bound, evaluations, warnflag, ladders)."""
    import scipy.optimize as sopt
    X, Z0 = so._2d(X), so._2d(Z0)
    m, d = Z0.shape
    nth = sg.n_theta(kid, d)
    count, ladders = [0], [0]

    def fg(x):
        count[0] += 1
        th = go.logexp(x[:nth])
        Zx = x[nth:].reshape(m, d) if optimize_z else Z0
        nll, g, gz, _, info = one_factor(kid, th, X, Y, Zx)
        if info != 0 or not (np.isfinite(nll) and np.all(np.isfinite(g)) and np.all(np.isfinite(gz))):
            ladders[0] += 1
            return 1e300, np.zeros_like(x)
        gx = g * -np.expm1(-th)
        return nll, np.concatenate([gx, gz.reshape(-1)]) if optimize_z else gx

    x0 = go.logexp_inv(np.asarray(theta0, dtype=np.float64))
    if optimize_z:
        x0 = np.concatenate([x0, Z0.reshape(-1)])
    x, fval, dct = sopt.fmin_l_bfgs_b(fg, x0, maxfun=max_evals, factr=factr)
    Zr = x[nth:].reshape(m, d) if optimize_z else Z0.copy()
    return go.logexp(x[:nth]), Zr, -fval, count[0], dct["warnflag"], ladders[0]
