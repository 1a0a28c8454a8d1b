"""Writes tests/golden/loo_mp_*.npz: leave-one-out cross-validation in 50-digit arithmetic (mpmath 1.3.0) on the samples and
theta of the three 50-digit fixtures that already exist (mp_rbfbrownian_n134, matern_mp_m32_n134, matern_mp_m52_n134).

    Ky = K + (sigma_n^2 + 1e-8) I (none of the three needs jitter), Kinv = Ky^-1 by LU with partial pivoting,
    loo_var_i = 1 / Kinv_ii,  loo_mean_i = y_i - (Kinv y)_i / Kinv_ii,  loo_lpd_i = log N(y_i; loo_mean_i, loo_var_i)

The kernels are written from their definitions here, as in gen_golden.py / gen_matern_golden.py; nothing of the engine or of
tests/loo_oracle.py is used, which is what tests/test_oracle_loo.py compares with these files.

    python tests/golden/gen_loo_golden.py"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = (("mp_rbfbrownian_n134", "loo_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_mp_m32_n134"),
         ("matern_mp_m52_n134", "loo_mp_m52_n134"))


def mp_loo(kid, theta, X, y):
    import mpmath as mp
    mp.mp.dps = 50
    N = len(y)
    x = [mp.mpf(float(v)) for v in X[:, 0]]
    yv = mp.matrix([mp.mpf(float(v)) for v in y])
    th = [mp.mpf(repr(float(v))) for v in theta]
    sn = th[-1]

    def k(a, b):
        if kid == 2:   # GPy RBF.K * Brownian.K for positive inputs: theta = (sigma_rbf^2, ell, sigma_b^2, sigma_n^2)
            return th[0] * mp.e ** (-(a - b) ** 2 / (2 * th[1] ** 2)) * th[2] * min(a, b)
        r = abs(a - b) / th[1]   # Matern, d = 1: theta = (sigma_f^2, ell, sigma_n^2)
        if kid == 3:
            s = mp.sqrt(3) * r
            return th[0] * (1 + s) * mp.e ** (-s)
        s = mp.sqrt(5) * r
        return th[0] * (1 + s + mp.mpf(5) / 3 * r * r) * mp.e ** (-s)

    Ky = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            Ky[i, j] = k(x[i], x[j])
        Ky[i, i] += sn + mp.mpf("1e-8")
    Kinv = mp.inverse(Ky)
    alpha = Kinv * yv
    mean, var, lpd = [], [], []
    for i in range(N):
        v = 1 / Kinv[i, i]
        m = yv[i] - alpha[i] * v
        mean.append(m)
        var.append(v)
        lpd.append(-mp.log(2 * mp.pi * v) / 2 - (yv[i] - m) ** 2 / (2 * v))
    f = lambda a: np.array([float(t) for t in a])
    return f(mean), f(var), f(lpd), float(sum(lpd))


def main():
    for src, dst in CASES:
        with np.load(os.path.join(OUT, src + ".npz"), allow_pickle=False) as z:
            kid, theta, X, y = int(z["kernel_id"]), z["theta"], z["X"], z["y"]
        assert X.shape[1] == 1 and kid in (2, 3, 4) and (kid != 2 or np.all(X > 0))
        mean, var, lpd, tot = mp_loo(kid, theta, X, y)
        np.savez_compressed(os.path.join(OUT, dst + ".npz"), source="mpmath", fixture=src, kernel_id=kid, theta=theta,
                            loo_mean=mean, loo_var=var, loo_lpd=lpd, lpd_sum=tot)
        print(dst, "lpd_sum", tot)


if __name__ == "__main__":
    main()
