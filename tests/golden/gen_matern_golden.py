#!/usr/bin/env python3
"""Generates the Matern fixtures tests/golden/matern_*.npz (needs scikit-learn and mpmath; run from a development checkout, the
tests only read what it wrote).  The fixtures are data: inputs, theta, expected outputs.  Nothing here uses oracle/ or
tests/matern_oracle.py for an expected value -- the sources are, per fixture `source` field:

  sklearn  matern_sk_m{32,52}_n{134_d1,256_d3,2048_d6}.npz -- scikit-learn GaussianProcessRegressor(optimizer=None, alpha=0) with
           ConstantKernel * Matern(length_scale=[...], nu=1.5 | 2.5) + WhiteKernel(sigma_n^2 + 1e-8) at fixed theta: mean and
           latent variance at Xs, alpha, logML and its gradient (log_marginal_likelihood(eval_gradient=True), converted from
           log to natural parameters: d/dtheta = (d/dlog theta) / theta).  The (134, 1) case is the reference-shaped window: the
           training part of the slip window stored in slipval_window_rbfbrownian.npz (raw tick counts) and the 599 ticks the
           node publishes; the others are seeded synthetic windows.
  closed   matern_closed_m{32,52}_n{1,2}.npz -- N = 1 and N = 2 in python floats: the 2 x 2 inverse and determinant written
           out, mean / latent variance at one test point, logML and its gradient (by the same dL/dK contraction, written out).
  mpmath   matern_mp_m{32,52}_n134.npz -- the (134, 1) window again in 50-digit arithmetic: kernel from its definition, LU with
           pivoting for the inverse and the determinant (no Cholesky, no numpy): mean, latent variance, logML, gradient.
  The jitter ladder is not exercised by any fixture (every matrix here is positive definite as it stands).
  Not written here: pre_matern_se_ard.npy and pre_matern_rbf_brownian.npy are every output of one SE_ARD batch / the reference's
  RBF x Brownian window (tests/test_gpu_matern.py legacy_outputs), recorded on an MI355X by `python tests/test_gpu_matern.py
  --record` with the library as it was BEFORE the Matern kernels were added; the library has to reproduce them bitwise.

Stored keys: source, kernel_id, theta, X, y, Xs, mean, var_latent, logml, dlogml_dtheta and, where cheap, alpha."""
import math
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
M32, M52 = 3, 4
EPS = 1e-8   # what exact inference adds to the diagonal besides the noise variance


def save(name, **kw):
    np.savez(os.path.join(OUT, name + ".npz"), **kw)
    print("wrote", name, {k: np.asarray(v).shape for k, v in kw.items() if np.asarray(v).ndim})


def slip_window():
    z = np.load(os.path.join(OUT, "slipval_window_rbfbrownian.npz"))
    t, s = z["time_array"], z["slip_array"]
    ntr = int(0.9 * len(t))
    X = t[:ntr, None].astype(np.float64)
    Xs = (t.min() + len(t) + np.arange(599.0))[:, None]
    return X, s[:ntr].astype(np.float64), Xs


def synth_window(seed, N, d, M):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, d))
    w = rng.normal(size=d)
    y = np.sin(X @ w) + 0.3 * np.cos(2.0 * X[:, 0]) + 0.05 * rng.normal(size=N)
    Xs = rng.uniform(-2.2, 2.2, (M, d))
    return X, y, Xs


def sklearn_case(name, kid, X, y, Xs, theta):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    theta = np.asarray(theta, dtype=np.float64)
    noise = theta[-1] + EPS
    kern = ConstantKernel(theta[0]) * Matern(length_scale=theta[1:-1], nu=1.5 if kid == M32 else 2.5) + WhiteKernel(noise)
    gpr = GaussianProcessRegressor(kern, alpha=0.0, optimizer=None).fit(X, y)
    mean, std = gpr.predict(Xs, return_std=True)
    lml, glog = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
    nat = np.concatenate([theta[:-1], [noise]])
    assert np.allclose(np.exp(gpr.kernel_.theta), nat, rtol=1e-12)
    save(name, source="sklearn", kernel_id=kid, theta=theta, X=X, y=y, Xs=Xs, mean=mean, var_latent=std ** 2 - noise,
         logml=float(lml), dlogml_dtheta=glog / nat, alpha=gpr.alpha_)


def k_float(kid, th, a, b):
    r2 = sum(((ai - bi) / l) ** 2 for ai, bi, l in zip(a, b, th[1:-1]))
    if kid == M32:
        s = math.sqrt(3.0 * r2)
        return th[0] * (1.0 + s) * math.exp(-s), -1.5 * th[0] * math.exp(-s)
    s = math.sqrt(5.0 * r2)
    return th[0] * (1.0 + s + 5.0 / 3.0 * r2) * math.exp(-s), -5.0 / 6.0 * th[0] * (1.0 + s) * math.exp(-s)


def closed_cases():
    for kid, tag in ((M32, "m32"), (M52, "m52")):
        # N = 1
        th, x, yv, xs = [1.3, 0.7, 0.05], [0.4], 0.9, [1.1]
        c = th[0] + th[2] + EPS
        ks, dks = k_float(kid, th, xs, x)
        # dlogML/dK = 0.5 (alpha^2 - 1/c); dK/dsigma_f^2 = 1, dK/dell = 0 (r = 0), dK/dsigma_n^2 = 1
        w = 0.5 * ((yv / c) ** 2 - 1.0 / c)
        save(f"matern_closed_{tag}_n1", source="closed", kernel_id=kid, theta=np.array(th), X=np.array([x]), y=np.array([yv]),
             Xs=np.array([xs]), mean=np.array([ks * yv / c]), var_latent=np.array([th[0] - ks * ks / c]),
             logml=-0.5 * yv * yv / c - 0.5 * math.log(c) - 0.5 * math.log(2.0 * math.pi), dlogml_dtheta=np.array([w, 0.0, w]),
             alpha=np.array([yv / c]))
        # N = 2, d = 2
        th = [0.8, 0.9, 2.5, 0.02]
        xa, xb, ya, yb, xs = [0.1, -0.3], [0.9, 0.6], 0.5, -0.2, [0.4, 0.2]
        a = th[0] + th[3] + EPS
        b, db = k_float(kid, th, xa, xb)
        det = a * a - b * b
        inv = [[a / det, -b / det], [-b / det, a / det]]
        al = [inv[0][0] * ya + inv[0][1] * yb, inv[1][0] * ya + inv[1][1] * yb]
        k1, _ = k_float(kid, th, xs, xa)
        k2, _ = k_float(kid, th, xs, xb)
        quad = k1 * (inv[0][0] * k1 + inv[0][1] * k2) + k2 * (inv[1][0] * k1 + inv[1][1] * k2)
        W = [[0.5 * (al[i] * al[j] - inv[i][j]) for j in range(2)] for i in range(2)]
        g = [W[0][0] + W[1][1] + 2.0 * W[0][1] * b / th[0]]
        for q in range(2):
            dq = xa[q] - xb[q]
            g.append(2.0 * W[0][1] * db * (-2.0 * dq * dq / th[1 + q] ** 3))
        g.append(W[0][0] + W[1][1])
        save(f"matern_closed_{tag}_n2", source="closed", kernel_id=kid, theta=np.array(th), X=np.array([xa, xb]),
             y=np.array([ya, yb]), Xs=np.array([xs]), mean=np.array([k1 * al[0] + k2 * al[1]]),
             var_latent=np.array([th[0] - quad]),
             logml=-0.5 * (ya * al[0] + yb * al[1]) - 0.5 * math.log(det) - math.log(2.0 * math.pi), dlogml_dtheta=np.array(g),
             alpha=np.array(al))


def mp_case(kid, tag, theta):
    import mpmath as mp
    mp.mp.dps = 50
    X, y, Xs = slip_window()
    N = len(y)
    x = [mp.mpf(float(v)) for v in X[:, 0]]
    yv = mp.matrix([mp.mpf(float(v)) for v in y])
    sf, ell, sn = (mp.mpf(repr(float(v))) for v in theta)

    def k(a, b):
        r = abs(a - b) / ell
        if kid == M32:
            s = mp.sqrt(3) * r
            return sf * (1 + s) * mp.e ** (-s), -mp.mpf(3) / 2 * sf * mp.e ** (-s)
        s = mp.sqrt(5) * r
        return sf * (1 + s + mp.mpf(5) / 3 * r * r) * mp.e ** (-s), -mp.mpf(5) / 6 * sf * (1 + s) * mp.e ** (-s)

    K, dK = mp.matrix(N, N), mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            K[i, j], dK[i, j] = k(x[i], x[j])
    Ky = K.copy()
    for i in range(N):
        Ky[i, i] += sn + mp.mpf("1e-8")
    Kinv = mp.inverse(Ky)                     # LU with partial pivoting
    alpha = Kinv * yv
    _, _, U = mp.lu(Ky)
    logdet = sum(mp.log(abs(U[i, i])) for i in range(N))
    logml = -(yv.T * alpha)[0] / 2 - logdet / 2 - mp.mpf(N) / 2 * mp.log(2 * mp.pi)
    mean, var = [], []
    for xsv in Xs[:, 0]:
        ks = mp.matrix([k(mp.mpf(float(xsv)), x[i])[0] for i in range(N)])
        mean.append(float((ks.T * alpha)[0]))
        var.append(float(sf - (ks.T * (Kinv * ks))[0]))
    g = [mp.mpf(0)] * 3
    for i in range(N):
        for j in range(N):
            w = (alpha[i] * alpha[j] - Kinv[i, j]) / 2
            g[0] += w * K[i, j] / sf
            g[1] += w * dK[i, j] * (-2 * (x[i] - x[j]) ** 2 / ell ** 3)
            if i == j:
                g[2] += w
    save(f"matern_mp_{tag}_n134", source="mpmath", kernel_id=kid, theta=np.asarray(theta, dtype=np.float64), X=X, y=y, Xs=Xs,
         mean=np.array(mean), var_latent=np.array(var), logml=float(logml), dlogml_dtheta=np.array([float(v) for v in g]),
         alpha=np.array([float(v) for v in alpha]))


SLIP_THETA = [0.05, 25.0, 0.002]


def main(what):
    if "closed" in what:
        closed_cases()
    if "sklearn" in what:
        for kid, tag in ((M32, "m32"), (M52, "m52")):
            X, y, Xs = slip_window()
            sklearn_case(f"matern_sk_{tag}_n134_d1", kid, X, y, Xs, SLIP_THETA)
            X, y, Xs = synth_window(11, 256, 3, 77)
            sklearn_case(f"matern_sk_{tag}_n256_d3", kid, X, y, Xs, [1.2, 0.8, 1.5, 2.2, 0.01])
            X, y, Xs = synth_window(12, 2048, 6, 150)
            sklearn_case(f"matern_sk_{tag}_n2048_d6", kid, X, y, Xs, [0.9, 1.4, 2.0, 1.1, 2.8, 1.7, 3.1, 0.02])
    if "mpmath" in what:
        mp_case(M32, "m32", SLIP_THETA)
        mp_case(M52, "m52", SLIP_THETA)


if __name__ == "__main__":
    main(sys.argv[1:] or ["closed", "sklearn", "mpmath"])
