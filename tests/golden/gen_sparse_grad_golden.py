#!/usr/bin/env python3
"""Writes tests/golden/sparse_grad_mp_k<kid>.npz: the gradient of the sparse (inducing-point) bound in theta and in the inducing
inputs Z for gen_sparse_golden.py's problems (N = 40, m = 7), by the DENSE N x N statement in mpmath at 50 digits:

    Q = K_fu (K_uu + 1e-8 I)^-1 K_uf      S = Q + sigma2 I      a = S^-1 y      sigma2 = sigma_n^2 + 1e-8
    F = log N(y | 0, S) - tr(K_ff - Q) / (2 sigma2)
    H = dF/dQ = (a a^T - S^-1) / 2 + I / (2 sigma2)
    dF/dK_uf = 2 K_uu^-1 K_uf H      dF/dK_uu = -K_uu^-1 K_uf H K_fu K_uu^-1      dF/dk(x_i, x_i) = -1 / (2 sigma2)
    dF/dsigma_n^2 = tr(a a^T - S^-1) / 2 + tr(K_ff - Q) / (2 sigma2^2)

The kernels are written from their definitions below and differentiated numerically at 50 digits (mpmath.diff) entry by entry:
nothing of the oracle or the engine is used.  The 1e-8 on K_uu's diagonal is a constant.

   python tests/golden/gen_sparse_grad_golden.py          (needs mpmath; the fixtures are committed, the tests do not)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import test_gpu_sparse as tg                # noqa: E402  (the problem generator of the GPU tests: inputs only)

mp.mp.dps = 50
N, m = 40, 7


def kernel(kid, th, a, b):
    """k(a, b) for a != b from the definitions: th the kernel's own parameters (no noise), a and b lists of mpf."""
    d = len(a)
    if kid == 2:
        rbf = th[0] * mp.exp(-(a[0] - b[0]) ** 2 / (2 * th[1] ** 2))
        same = mp.sign(a[0]) == mp.sign(b[0])
        return rbf * (th[2] * min(abs(a[0]), abs(b[0])) if same else 0)
    ell = [th[1]] * d if kid == 0 else th[1:1 + d]
    r2 = sum(((a[q] - b[q]) / ell[q]) ** 2 for q in range(d))
    if kid <= 1:
        return th[0] * mp.exp(-r2 / 2)
    s = mp.sqrt((3 if kid == 3 else 5) * r2)
    return th[0] * ((1 + s) * mp.exp(-s) if kid == 3 else (1 + s + 5 * r2 / 3) * mp.exp(-s))


def kdiag(kid, th, a):
    return th[0] * th[2] * abs(a[0]) if kid == 2 else th[0]


def matrices(kid, th, X, Z):
    Kuu = mp.matrix(m, m)
    for r in range(m):
        for s in range(m):
            Kuu[r, s] = kdiag(kid, th, Z[r]) + mp.mpf("1e-8") if r == s else kernel(kid, th, Z[r], Z[s])
    Kuf = mp.matrix(m, N)
    for r in range(m):
        for i in range(N):
            Kuf[r, i] = kernel(kid, th, Z[r], X[i])
    kff = [kdiag(kid, th, X[i]) for i in range(N)]
    return Kuu, Kuf, kff


def dense_gradient(kid, theta, Xf, yf, Zf):
    d = Xf.shape[1]
    mpl = lambda v: [mp.mpf(float(x)) for x in v]
    th, X, Z, y = mpl(theta[:-1]), [mpl(r) for r in Xf], [mpl(r) for r in Zf], mp.matrix(mpl(yf))
    sigma2 = mp.mpf(float(theta[-1])) + mp.mpf("1e-8")
    Kuu, Kuf, kff = matrices(kid, th, X, Z)
    Kinv = mp.inverse(Kuu)
    Q = Kuf.T * Kinv * Kuf
    S = Q + sigma2 * mp.eye(N)
    Sinv = mp.inverse(S)
    a = Sinv * y
    L = mp.cholesky(S)
    trace = sum(kff[i] - Q[i, i] for i in range(N))
    bound = (-mp.mpf(N) / 2 * mp.log(2 * mp.pi) - sum(mp.log(L[i, i]) for i in range(N)) - (y.T * a)[0, 0] / 2 - trace / (2 * sigma2))
    H = (a * a.T - Sinv) / 2 + mp.eye(N) / (2 * sigma2)
    Guf = 2 * Kinv * Kuf * H
    Guu = -Kinv * Kuf * H * Kuf.T * Kinv
    gdiag = -1 / (2 * sigma2)
    nk = len(th)
    grad = []
    for p in range(nk):     # entry by entry: the derivative of each kernel value in theta_p at 50 digits
        def at(t, fn):
            tt = list(th)
            tt[p] = t
            return fn(tt)
        g = mp.mpf(0)
        for r in range(m):
            for s in range(m):
                fn = (lambda tt: kdiag(kid, tt, Z[r])) if r == s else (lambda tt: kernel(kid, tt, Z[r], Z[s]))
                g += Guu[r, s] * mp.diff(lambda t: at(t, fn), th[p])
            for i in range(N):
                g += Guf[r, i] * mp.diff(lambda t: at(t, lambda tt: kernel(kid, tt, Z[r], X[i])), th[p])
        for i in range(N):
            g += gdiag * mp.diff(lambda t: at(t, lambda tt: kdiag(kid, tt, X[i])), th[p])
        grad.append(g)
    grad.append(sum(a[i] ** 2 - Sinv[i, i] for i in range(N)) / 2 + trace / (2 * sigma2 ** 2))
    gradZ = np.zeros((m, d))
    for r in range(m):
        for q in range(d):
            def moved(t):
                z = list(Z[r])
                z[q] = t
                return z
            g = Guu[r, r] * mp.diff(lambda t: kdiag(kid, th, moved(t)), Z[r][q])
            for s in range(m):
                if s != r:   # entries (r, s) and (s, r) of the symmetric K_uu
                    g += (Guu[r, s] + Guu[s, r]) * mp.diff(lambda t: kernel(kid, th, moved(t), Z[s]), Z[r][q])
            for i in range(N):
                g += Guf[r, i] * mp.diff(lambda t: kernel(kid, th, moved(t), X[i]), Z[r][q])
            gradZ[r, q] = float(-g)
    return float(bound), np.array([float(-g) for g in grad]), gradZ


if __name__ == "__main__":
    for kid in range(5):
        d = 1 if kid == 2 else 2
        X, y, Z, _, theta = tg.problem(1, N, d, 9, m, kid, 700 + kid)
        bound, grad, gradZ = dense_gradient(kid, theta[0], X[0], y[0], Z[0])
        path = os.path.join(HERE, f"sparse_grad_mp_k{kid}.npz")
        np.savez(path, kid=kid, theta=theta[0], X=X[0], y=y[0], Z=Z[0], bound=bound, grad=grad, gradZ=gradZ, source="mpmath")
        print(path, "bound", bound, "grad", grad)
