#!/usr/bin/env python3
"""Writes tests/golden/sparse_mp_k<kid>.npz: the sparse (inducing-point) bound and forecast of one small problem per kernel,
N = 40, m = 7, M = 9, by the DENSE N x N statement -- a different algebraic route from tests/sparse_oracle.py's B = I + A form --
evaluated with mpmath at 50 digits on the oracle's kernel matrices:

    Q_ab = K_au (K_uu + 1e-8 I)^-1 K_ub          S = Q_ff + sigma2 I
    bound = log N(y | 0, S) - tr(K_ff - Q_ff) / (2 sigma2)
    mean = Q_*f S^-1 y          var = k_** - diag(Q_*f S^-1 Q_f*)          (the DTC predictive, by Woodbury the same as the oracle's)

   python tests/golden/gen_sparse_golden.py          (needs mpmath; the fixtures are committed, the tests do not)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from oracle import gp_oracle as go          # noqa: E402
import matern_oracle as mo                  # noqa: E402
import test_gpu_sparse as tg                # noqa: E402  (the problem generator of the GPU tests)

mp.mp.dps = 50
N, M, m = 40, 9, 7


def dense_statement(kid, theta, X, y, Z, Xs):
    o = mo if kid >= 3 else go
    M_ = lambda a: mp.matrix(np.asarray(a, dtype=np.float64).tolist())
    Kuu = M_(o.kernel_K(kid, theta, Z)) + mp.mpf("1e-8") * mp.eye(len(Z))
    Kuf, Kus = M_(o.kernel_K(kid, theta, Z, X)), M_(o.kernel_K(kid, theta, Z, Xs))
    kff, kss = o.kernel_Kdiag(kid, theta, X), o.kernel_Kdiag(kid, theta, Xs)
    sigma2 = mp.mpf(float(theta[-1])) + mp.mpf("1e-8")
    Kinv = mp.inverse(Kuu)
    Qff, Qsf = Kuf.T * Kinv * Kuf, Kus.T * Kinv * Kuf
    S = Qff + sigma2 * mp.eye(len(X))
    L = mp.cholesky(S)
    yv = M_(np.asarray(y)[:, None])
    Sinv = mp.inverse(S)
    Sinv_y = Sinv * yv
    logdet = 2 * sum(mp.log(L[i, i]) for i in range(len(X)))
    trace = sum(mp.mpf(float(kff[i])) - Qff[i, i] for i in range(len(X)))
    bound = -mp.mpf(len(X)) / 2 * mp.log(2 * mp.pi) - logdet / 2 - (yv.T * Sinv_y)[0, 0] / 2 - trace / (2 * sigma2)
    mean = Qsf * Sinv_y
    Sinv_Qfs = Sinv * Qsf.T
    var = [mp.mpf(float(kss[j])) - sum(Qsf[j, i] * Sinv_Qfs[i, j] for i in range(len(X))) for j in range(len(Xs))]
    return np.array([float(v) for v in mean]), np.array([float(v) for v in var]), float(bound)


if __name__ == "__main__":
    for kid in range(5):
        d = 1 if kid == 2 else 2
        X, y, Z, Xs, theta = tg.problem(1, N, d, M, m, kid, 700 + kid)
        mean, var, bound = dense_statement(kid, theta[0], X[0], y[0], Z[0], Xs[0])
        path = os.path.join(HERE, f"sparse_mp_k{kid}.npz")
        np.savez(path, kid=kid, theta=theta[0], X=X[0], y=y[0], Z=Z[0], Xs=Xs[0], mean=mean, var=var, bound=bound,
                 source="mpmath")
        print(path, "bound", bound)
