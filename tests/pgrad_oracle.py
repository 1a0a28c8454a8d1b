"""float64 oracle of the predictive gradients (cgp_fit_predict_grad_batch, cgp_predict_gradients): d mean / d x* and
d var / d x* at the test points, on the oracle's own factorisation (oracle/gp_oracle.py for ids 0, 1, 2; tests/matern_oracle.py
for ids 3, 4).  numpy / scipy only, the formulas of include/corenav_gp.h ("predictive gradients"):

    alpha = Ky^-1 y        B = Ky^-1 K(X, Xs)
    dmean[m][q] =                     sum_i dk(x*_m, x_i)/dx*_q alpha_i
    dvar [m][q] = dk(x*_m, x*_m)/dx*_q - 2 sum_i dk(x*_m, x_i)/dx*_q B[i][m]

the gradient of the UNCLIPPED variance without the noise term.  With r^2 = sum_q ((x*_q - x_iq) / ell_q)^2 and g = -2 dk/dr^2:
ids 0 / 1 / 3 / 4: dk/dx*_q = g (x_iq - x*_q) / ell_q^2, dk**/dx* = 0.  Id 2 (RBF x Brownian, d = 1):
    dk/dx* = R W (x_i - x*) / ell^2 + R sigma_b^2 sign(x*) [|x*| < |x_i| and equal signs],   dk**/dx* = sigma_r^2 sigma_b^2 sign(x*)
with sign(0) = 0 and the bracket 0 at a tie |x*| = |x_i|."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo


def _as2d(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def fit(kernel_id, theta, X, y):
    return mo.fit(kernel_id, theta, X, y) if kernel_id in mo.KERNELS else go.fit(kernel_id, theta, X, y)


def predict(f, Xs, include_noise=False):
    return mo.predict(f, Xs, include_noise) if f.kernel_id in mo.KERNELS else go.predict(f, Xs, include_noise)


def kernel_K(kernel_id, theta, X, X2):
    return mo.kernel_K(kernel_id, theta, X, X2) if kernel_id in mo.KERNELS else go.kernel_K(kernel_id, theta, X, X2)


def dK_dxs(kernel_id, theta, X, Xs):
    """dk(x*_m, x_i)/dx*_q as (N, M, d), and dk(x*_m, x*_m)/dx*_q as (M, d)."""
    theta = np.asarray(theta, dtype=np.float64)
    X, Xs = _as2d(X), _as2d(Xs)
    N, d = X.shape
    M = len(Xs)
    if kernel_id == go.KERNEL_RBF_BROWNIAN:
        x, xs = X[:, 0][:, None], Xs[:, 0][None, :]          # (N, 1), (1, M)
        ell = theta[1]
        R = theta[0] * np.exp(-0.5 * ((xs - x) / ell) ** 2)
        same = np.sign(x) == np.sign(xs)
        W = np.where(same, theta[2] * np.fmin(np.abs(x), np.abs(xs)), 0.0)
        br = np.where(same & (np.abs(xs) < np.abs(x)), theta[2] * np.sign(xs), 0.0)
        dk = R * W * (x - xs) / ell ** 2 + R * br
        return dk[:, :, None], (theta[0] * theta[2] * np.sign(Xs[:, 0]))[:, None]
    ell = np.full(d, theta[1]) if kernel_id == go.KERNEL_SE_ISO else np.asarray(theta[1:1 + d])
    D = (X[:, None, :] - Xs[None, :, :]) / ell[None, None, :]       # (x_i - x*) / ell, (N, M, d)
    r2 = np.sum(D * D, axis=2)
    if kernel_id in mo.KERNELS:
        g = -2.0 * theta[0] * mo.radial(kernel_id, r2)[1]
    else:
        g = theta[0] * np.exp(-0.5 * r2)
    return g[:, :, None] * D / ell[None, None, :], np.zeros((M, d))


def predictive_gradients(f, Xs):
    """(dmean, dvar), each (M, d), of the fit f (a go.Fit) at Xs."""
    Xs = _as2d(Xs)
    dk, dkss = dK_dxs(f.kernel_id, f.theta, f.X, Xs)
    Ks = kernel_K(f.kernel_id, f.theta, f.X, Xs)
    B = sla.cho_solve((f.L, True), Ks)                               # (N, M)
    dmean = np.einsum("imq,i->mq", dk, f.alpha)
    dvar = dkss - 2.0 * np.einsum("imq,im->mq", dk, B)
    return dmean, dvar


def unclipped_mean_var(f, Xs):
    """mean and the UNCLIPPED latent variance at Xs: what the gradients are the derivatives of."""
    Xs = _as2d(Xs)
    Ks = kernel_K(f.kernel_id, f.theta, f.X, Xs)
    V = sla.solve_triangular(f.L, Ks, lower=True)
    if f.kernel_id in mo.KERNELS:
        kss = mo.kernel_Kdiag(f.kernel_id, f.theta, Xs)
    else:
        kss = go.kernel_Kdiag(f.kernel_id, f.theta, Xs)
    return Ks.T @ f.alpha, kss - np.sum(V * V, 0)
