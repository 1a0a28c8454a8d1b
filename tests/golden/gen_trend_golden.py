#!/usr/bin/env python3
"""Generates tests/golden/trend_mp_*.npz: the pins of tests/trend_oracle.py (needs mpmath; a few seconds per case).

Each fixture holds one small problem (X, Y, H, Xs, Hs, theta, kernel id; basis [1, u, u^2][:q], u = (x0 - c) / s) and two sets of
expected values, both in 50-digit arithmetic with the kernel from its definition and LU with pivoting -- no Cholesky, no numpy,
nothing of oracle/:
  closed_*  the closed form of Rasmussen & Williams 2.7 (eqs. 2.41, 2.42, 2.45 in the vague-prior limit), written with Ky^-1
            itself: beta = (H Ky^-1 H^T)^-1 H Ky^-1 y, mean = k*^T Ky^-1 y + R^T beta, R = hs - H Ky^-1 k*,
            var = k** - k*^T Ky^-1 k* + R^T (H Ky^-1 H^T)^-1 R, logml = -1/2 y^T Ky^-1 y + 1/2 y^T C y - 1/2 log|Ky| - 1/2 log|A|
            - (N - q)/2 log 2 pi
  limit_*   the ZERO-MEAN GP with kernel k + b^2 h(x)^T h(x') at b^2 = 1e12 -- no trend formula at all -- with
            logml + q/2 log(2 pi b^2); it converges to the closed form like 1 / b^2
(H here is (q, N), as the C ABI lays it out.)  var includes sigma_n^2 (include_noise)."""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corenav_gp_amd.synth as synth  # noqa: E402
from trend_oracle import basis  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
mp.mp.dps = 50
B2 = mp.mpf(10) ** 12


def kern(kid, theta, a, b):
    """k(a, b) for one pair of inputs (lists of mpf), ids 0 (SE-iso), 1 (SE-ARD), 2 (RBF x Brownian)."""
    d = len(a)
    if kid == 2:
        x, y = a[0], b[0]
        same = (x > 0 and y > 0) or (x < 0 and y < 0)
        brown = theta[2] * min(abs(x), abs(y)) if same else mp.mpf(0)
        return theta[0] * mp.exp(-(x - y) ** 2 / (2 * theta[1] ** 2)) * brown
    ells = [theta[1]] * d if kid == 0 else theta[1:1 + d]
    return theta[0] * mp.exp(-sum(((a[i] - b[i]) / ells[i]) ** 2 for i in range(d)) / 2)


def solve_case(kid, theta, X, Y, H, Xs, Hs):
    th = [mp.mpf(float(t)) for t in theta]
    Xm = [[mp.mpf(float(v)) for v in row] for row in X]
    Xsm = [[mp.mpf(float(v)) for v in row] for row in Xs]
    N, M, P, q = len(X), len(Xs), len(Y), len(H)
    noise = th[-1]
    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            K[i, j] = kern(kid, th, Xm[i], Xm[j])
    Ks = mp.matrix(N, M)
    for i in range(N):
        for m in range(M):
            Ks[i, m] = kern(kid, th, Xm[i], Xsm[m])
    kss = [kern(kid, th, Xsm[m], Xsm[m]) for m in range(M)]
    Hm = mp.matrix([[mp.mpf(float(v)) for v in row] for row in H])        # (q, N)
    Hsm = mp.matrix([[mp.mpf(float(v)) for v in row] for row in Hs])      # (q, M)
    Ym = mp.matrix([[mp.mpf(float(v)) for v in row] for row in Y]).T      # (N, P)
    eye = mp.eye(N)
    log2pi = mp.log(2 * mp.pi)

    # closed form
    Ky = K + (noise + mp.mpf("1e-8")) * eye
    Kyi = mp.inverse(Ky)
    A = Hm * Kyi * Hm.T
    Ai = mp.inverse(A)
    beta = Ai * (Hm * Kyi * Ym)                       # (q, P)
    R = Hsm - Hm * Kyi * Ks                           # (q, M)
    mean = (Ks.T * Kyi * Ym).T + beta.T * R           # (P, M)
    RAR = R.T * Ai * R
    KKK = Ks.T * Kyi * Ks
    var = [kss[m] - KKK[m, m] + RAR[m, m] + noise for m in range(M)]
    C = Kyi * Hm.T * Ai * Hm * Kyi
    yKy, yCy = Ym.T * Kyi * Ym, Ym.T * C * Ym
    logml = [-yKy[p, p] / 2 + yCy[p, p] / 2 - mp.log(mp.det(Ky)) / 2 - mp.log(mp.det(A)) / 2 - (N - q) * log2pi / 2 for p in range(P)]
    closed = dict(mean=mean, var=var, beta=beta.T, logml=logml)

    # large-prior limit: a zero-mean GP with kernel k + b^2 h h'^T
    Kb = Ky + B2 * (Hm.T * Hm)
    Kbi = mp.inverse(Kb)
    Ksb = Ks + B2 * (Hm.T * Hsm)
    lmean = (Ksb.T * Kbi * Ym).T
    KbK = Ksb.T * Kbi * Ksb
    HsHs = Hsm.T * Hsm
    lvar = [kss[m] + B2 * HsHs[m, m] - KbK[m, m] + noise for m in range(M)]
    yKby = Ym.T * Kbi * Ym
    llogml = [-yKby[p, p] / 2 - mp.log(mp.det(Kb)) / 2 - N * log2pi / 2 + q * mp.log(2 * mp.pi * B2) / 2 for p in range(P)]
    # beta of the limit: the posterior mean of the weights, b^2 H Kb^-1 y
    lbeta = (B2 * Hm * Kbi * Ym).T
    limit = dict(mean=lmean, var=lvar, beta=lbeta, logml=llogml)

    def arr(v, shape):
        return np.array([float(x) for x in v], dtype=np.float64).reshape(shape)

    out = {}
    for tag, r in (("closed", closed), ("limit", limit)):
        out[tag + "_mean"] = arr(r["mean"], (P, M))
        out[tag + "_var"] = arr(r["var"], (M,))
        out[tag + "_beta"] = arr(r["beta"], (P, q))
        out[tag + "_logml"] = arr(r["logml"], (P,))
    return out


def case(name, kid, d, N, M, P, q, seed):
    rng = np.random.default_rng(seed)
    if kid == 2:   # a window of the reference's kind: ticks, slip series with an offset and a drift
        t = np.arange(11, 11 + N, dtype=np.float64)
        X = t[:, None]
        Xs = (t[-1] + 1.0 + 3.0 * np.arange(M, dtype=np.float64))[:, None]
        Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1)), t) + 0.1 + 0.002 * p * (t - t[0]) for p in range(P)])
        theta = np.array([0.5, 30.0, 0.01, 0.002])
    else:
        X = np.sort(rng.uniform(0.0, 10.0, size=(N, d)), axis=0) if d == 1 else rng.uniform(0.0, 10.0, size=(N, d))
        Xs = rng.uniform(-1.0, 12.0, size=(M, d))
        Y = np.stack([np.sin(X[:, 0] + p) + 0.3 * (p + 1) * X[:, 0] - 1.0 + 0.1 * rng.normal(size=N) for p in range(P)])
        theta = np.array([1.0, 1.5, 0.01]) if kid == 0 else np.concatenate([[1.0], np.linspace(1.2, 2.4, d), [0.01]])
    c, s = float(np.mean(X[:, 0])), float(np.std(X[:, 0]))
    H, Hs = basis(X[:, 0], c, s, q), basis(Xs[:, 0], c, s, q)
    out = solve_case(kid, theta, X, Y, H, Xs, Hs)
    np.savez(os.path.join(OUT, name + ".npz"), kid=kid, theta=theta, X=X, Y=Y, H=H, Xs=Xs, Hs=Hs, b2=float(B2), source="mpmath", **out)
    em = np.max(np.abs(out["closed_mean"] - out["limit_mean"])) / np.max(np.abs(out["closed_mean"]))
    el = np.max(np.abs(out["closed_logml"] - out["limit_logml"]) / np.maximum(1.0, np.abs(out["closed_logml"])))
    print(f"{name}: closed form vs large-prior limit in 50 digits: mean {em:.2e} logml {el:.2e}")


if __name__ == "__main__":
    case("trend_mp_se1_q2", 0, 1, 40, 5, 2, 2, 1)
    case("trend_mp_ard3_q3", 1, 3, 50, 5, 2, 3, 2)
    case("trend_mp_brown_q2", 2, 1, 60, 5, 2, 2, 3)
