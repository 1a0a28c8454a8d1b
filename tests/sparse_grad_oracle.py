"""Oracle of the sparse fits' objective (cgp_sparse_nll_grad_batch, cgp_optimize_sparse_batch): the gradient of the collapsed
variational bound of tests/sparse_oracle.py in theta (natural parameters, cgp_nll_grad's order) and in the inducing inputs Z, in
closed form on sparse_oracle's quantities, and scipy's L-BFGS-B over Logexp(theta) and free Z in the manner of
multi_opt_oracle.optimize_multi.  With F the bound, sigma2 = sigma_n^2 + 1e-8, K_uu = L_u L_u^T, B = I + A = L_B L_B^T:
    chat = L_B^-T c      Q = I - B^-1 - chat chat^T      mu = L_u^-T chat
    T = L_u^-T Q L_u^-1 / (2 sigma2) = dF/dPhi      G_uu = 1/2 L_u^-T (Q - A) L_u^-1 = dF/dK_uu      R = 2 T K_uf + mu y^T / sigma2 = dF/dK_uf
The 1e-8 and any jitter on K_uu's diagonal are constants of the evaluation.  The kernels' derivatives are written out here; ties of
the Brownian factor (|z| = |x|) take k_pgrad_contract's convention: the derivative in z is that of min(|z|, |x|) for |z| < |x| only."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import sparse_oracle as so


def n_theta(kid, d):
    return so._mod(kid).n_theta(kid, d)


def kernel_parts(kid, theta, A, B, same=False):
    """K(A, B) (a x b), [dK/dtheta_p] for the kernel's own parameters (the noise is not one), dK/dA (a x b x d: the derivative of
    entry (i, j) in the coordinates of A's point i, B held fixed).  same: B is A, and the diagonal is k(z, z)."""
    theta = np.asarray(theta, dtype=np.float64)
    A, B = so._2d(A), so._2d(B)
    d = A.shape[1]
    D = A[:, None, :] - B[None, :, :]
    if kid in (0, 1, 3, 4):
        ell = np.full(d, theta[1]) if kid == 0 else np.asarray(theta[1:1 + d])
        S = D / ell
        r2 = np.sum(S * S, axis=2)
        if kid <= 1:
            f, fp = np.exp(-0.5 * r2), -0.5 * np.exp(-0.5 * r2)
        else:
            import matern_oracle as mo
            f, fp = mo.radial(kid, r2)
        K = theta[0] * f
        dl = [theta[0] * fp * (-2.0 * S[:, :, q] ** 2 / ell[q]) for q in range(d)]
        dth = [f] + ([sum(dl)] if kid == 0 else dl)
        dA = theta[0] * fp[:, :, None] * 2.0 * S / ell
        return K, dth, dA
    assert kid == 2 and d == 1
    a, b = A[:, 0][:, None], B[:, 0][None, :]
    rbf = np.exp(-0.5 * (a - b) ** 2 / theta[1] ** 2)
    samesign = np.sign(a) == np.sign(b)
    w = np.where(samesign, np.fmin(np.abs(a), np.abs(b)), 0.0)
    K = theta[0] * theta[2] * rbf * w
    dmin = np.where(samesign & (np.abs(a) < np.abs(b)), np.sign(a), 0.0) * np.ones_like(b)
    if same:
        dmin[np.diag_indices(len(A))] = np.sign(A[:, 0])      # d k(z, z) / dz = s_r^2 s_b^2 sign z
    dA = (-K * (a - b) / theta[1] ** 2 + theta[0] * theta[2] * rbf * dmin)[:, :, None]
    return K, [K / theta[0], K * (a - b) ** 2 / theta[1] ** 3, K / theta[2]], dA


def diag_parts(kid, theta, X):
    """[d k(x_i, x_i) / dtheta_p] (N,) for the kernel's own parameters."""
    X = so._2d(X)
    N, d = X.shape
    if kid == 2:
        ax = np.abs(X[:, 0])
        return [theta[2] * ax, np.zeros(N), theta[0] * ax]
    return [np.ones(N)] + [np.zeros(N)] * (n_theta(kid, d) - 2)


def nll_grad(kid, theta, X, y, Z, jitter=0.0, eps=1e-8):
    """-> (nll = -bound, d nll / d theta (nth,), d nll / d Z (m, d), info).  jitter: added to K_uu's diagonal beside eps, a constant.
    No ladder here: a K_uu or B that does not factor gives info != 0 and NaN."""
    theta = np.asarray(theta, dtype=np.float64)
    X, Z = so._2d(X), so._2d(Z)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, m, d = len(X), len(Z), X.shape[1]
    nth = n_theta(kid, d)
    sigma2 = float(theta[-1]) + so.DIAG_EPS
    nan = (np.nan, np.full(nth, np.nan), np.full((m, d), np.nan))
    Kuu, dKuu, dKuu_z = kernel_parts(kid, theta, Z, Z, same=True)
    Lu, bad = so._first_bad_pivot(Kuu + (eps + jitter) * np.eye(m))
    if bad:
        return nan + (bad,)
    Kuf, dKuf, dKuf_z = kernel_parts(kid, theta, Z, X)
    Phi, b = Kuf @ Kuf.T, Kuf @ y
    kd = so._mod(kid).kernel_Kdiag(kid, theta, X)
    t = float(np.sum(kd))
    Li = sla.solve_triangular(Lu, np.eye(m), lower=True)
    A = Li @ Phi @ Li.T / sigma2
    A = 0.5 * (A + A.T)
    LB, bad = so._first_bad_pivot(np.eye(m) + A)
    if bad:
        return nan + (m + bad,)
    c = sla.solve_triangular(LB, Li @ b, lower=True) / sigma2
    bound = float(-0.5 * N * so.LOG_2PI - 0.5 * N * np.log(sigma2) - np.sum(np.log(np.diag(LB))) - y @ y / (2.0 * sigma2)
                  + 0.5 * c @ c - t / (2.0 * sigma2) + 0.5 * np.trace(A))
    LBi = sla.solve_triangular(LB, np.eye(m), lower=True)
    Binv = LBi.T @ LBi
    chat = LBi.T @ c
    Q = np.eye(m) - Binv - np.outer(chat, chat)
    mu = Li.T @ chat
    T = Li.T @ Q @ Li / (2.0 * sigma2)
    Guu = 0.5 * Li.T @ (Q - A) @ Li
    R = 2.0 * T @ Kuf + np.outer(mu, y) / sigma2
    dF = np.zeros(nth)
    for p, (duu, duf, dd) in enumerate(zip(dKuu, dKuf, diag_parts(kid, theta, X))):
        dF[p] = np.sum(Guu * duu) + np.sum(R * duf) - np.sum(dd) / (2.0 * sigma2)
    dF[nth - 1] = (-N + (y @ y + t) / sigma2 - np.trace(A) + m - np.trace(Binv) - c @ c - chat @ chat) / (2.0 * sigma2)
    off = Guu - np.diag(np.diag(Guu))
    dZ = (np.einsum("ri,riq->rq", R, dKuf_z) + 2.0 * np.einsum("rs,rsq->rq", off, dKuu_z)
          + np.diag(Guu)[:, None] * dKuu_z[np.arange(m), np.arange(m), :])
    return -bound, -dF, -dZ, 0


def nll_grad_ladder(kid, theta, X, y, Z):
    """The host form: the evaluation at the first jitter of sparse_oracle's ladder at which K_uu factors (0 first).
    -> (nll, grad, gradZ, info, steps, jitter)."""
    out = nll_grad(kid, theta, X, y, Z)
    if out[3] == 0 or out[3] > len(so._2d(Z)):
        return out + (0, 0.0)
    for k, jit in enumerate(so.ladder_jitters(kid, theta, Z)):
        out = nll_grad(kid, theta, X, y, Z, jitter=jit)
        if out[3] == 0:
            break
    return out + (k + 1, jit)


def optimize_sparse(kid, X, y, Z0, theta0, optimize_z, max_evals=1000, factr=1e7):
    """SparseGPRegression(...).optimize(): scipy L-BFGS-B without bounds over [Logexp^-1(theta) | Z row-major] (Z only when
    optimize_z), pgtol 1e-5.  A trial point that does not factor without the ladder is infeasible (the compared cases never need a
    ladder step: `ladders` counts the points that would have).  -> (theta, Z, bound, evaluations, warnflag, ladders)."""
    import scipy.optimize as sopt
    X, Z0 = so._2d(X), so._2d(Z0)
    m, d = Z0.shape
    nth = n_theta(kid, d)
    count, ladders = [0], [0]

    def fg(x):
        count[0] += 1
        th = go.logexp(x[:nth])
        Zx = x[nth:].reshape(m, d) if optimize_z else Z0
        nll, g, gz, info = nll_grad(kid, th, X, y, Zx)
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
