#!/usr/bin/env python3
"""Generates the predictive-gradient pins tests/golden/pgrad_mp_{rbfbrownian,m32,m52}_n134.npz (needs mpmath; run from a
development checkout, the suite only reads the files): the N = 134 slipVal window (slipval_window_rbfbrownian.npz, first 90 % of
the ticks) in 50-digit arithmetic, every formula from its definition -- kernel and its derivative with respect to the test input
written out per kernel, Ky^-1 by LU with partial pivoting, no Cholesky, no shared code with tests/pgrad_oracle.py:
    dmean[m] = sum_i dk(x*_m, x_i)/dx* alpha_i        dvar[m] = dk(x*_m, x*_m)/dx* - 2 sum_i dk(x*_m, x_i)/dx* (Ky^-1 k*_m)_i
Test points: 24 ticks after the window (the reference's grid), 12 points inside the window off the ticks, and for
RBF x Brownian 4 ticks OF the window (ties |x*| = |x_i|: the bracket of the header's formula is 0 there, by convention).
   python tests/golden/gen_pgrad_golden.py"""
import os
import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = [(2, "rbfbrownian", [0.5, 30.0, 0.01, 0.002]), (3, "m32", [0.05, 25.0, 0.002]), (4, "m52", [0.05, 25.0, 0.002])]


def slip_window(kid):
    z = np.load(os.path.join(OUT, "slipval_window_rbfbrownian.npz"))
    t, s = z["time_array"], z["slip_array"]
    ntr = int(0.9 * len(t))
    X = t[:ntr].astype(np.float64)
    rng = np.random.default_rng(134)
    inside = X[rng.integers(0, ntr - 1, size=12)] + np.round(rng.uniform(0.1, 0.9, size=12), 3)
    pts = [X[-1] + 1.0 + np.arange(24.0), inside]
    if kid == 2:
        pts.append(X[[3, 40, 77, 133]])
    return X, s[:ntr].astype(np.float64), np.concatenate(pts)


def mp_case(kid, tag, theta):
    import mpmath as mp
    mp.mp.dps = 50
    X, y, Xs = slip_window(kid)
    N = len(y)
    x = [mp.mpf(float(v)) for v in X]
    yv = mp.matrix([mp.mpf(float(v)) for v in y])
    th = [mp.mpf(repr(float(v))) for v in theta]
    sgn = lambda v: mp.mpf(1) if v > 0 else (mp.mpf(-1) if v < 0 else mp.mpf(0))

    def k(a, b):
        """k(a, b) and dk/da"""
        if kid == 2:
            sr, ell, sb = th[0], th[1], th[2]
            R = sr * mp.e ** (-(a - b) ** 2 / (2 * ell ** 2))
            same = sgn(a) == sgn(b)
            W = sb * min(abs(a), abs(b)) if same else mp.mpf(0)
            dW = sb * sgn(a) if (same and abs(a) < abs(b)) else mp.mpf(0)   # a tie: 0
            return R * W, R * W * (b - a) / ell ** 2 + R * dW
        sf, ell = th[0], th[1]
        r = abs(a - b) / ell
        s = (mp.sqrt(3) if kid == 3 else mp.sqrt(5)) * r
        if kid == 3:
            return sf * (1 + s) * mp.e ** (-s), 3 * sf * mp.e ** (-s) * (b - a) / ell ** 2
        return sf * (1 + s + mp.mpf(5) / 3 * r * r) * mp.e ** (-s), mp.mpf(5) / 3 * sf * (1 + s) * mp.e ** (-s) * (b - a) / ell ** 2

    Ky = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            Ky[i, j] = k(x[i], x[j])[0]
        Ky[i, i] += th[-1] + mp.mpf("1e-8")
    Kinv = mp.inverse(Ky)
    alpha = Kinv * yv
    dmean, dvar, mean, var = [], [], [], []
    for xsv in Xs:
        a = mp.mpf(float(xsv))
        kd = [k(a, x[i]) for i in range(N)]
        ks, dks = mp.matrix([v[0] for v in kd]), mp.matrix([v[1] for v in kd])
        b = Kinv * ks
        kss, dkss = (th[0] * th[2] * abs(a), th[0] * th[2] * sgn(a)) if kid == 2 else (th[0], mp.mpf(0))
        mean.append(float((ks.T * alpha)[0]))
        var.append(float(kss - (ks.T * b)[0]))
        dmean.append(float((dks.T * alpha)[0]))
        dvar.append(float(dkss - 2 * (dks.T * b)[0]))
    name = f"pgrad_mp_{tag}_n134"
    np.savez(os.path.join(OUT, name + ".npz"), source="mpmath", kernel_id=kid, theta=np.asarray(theta, dtype=np.float64), X=X[:, None],
             y=y, Xs=Xs[:, None], mean=np.array(mean), var_latent=np.array(var), dmean=np.array(dmean)[:, None],
             dvar=np.array(dvar)[:, None])
    print("wrote", name)


if __name__ == "__main__":
    for case in CASES:
        mp_case(*case)
