"""Writes tests/golden/loo_grad_mp_*.npz: the leave-one-out objective nlpd = -lpd_sum and its gradient with respect to the natural
parameters in 50-digit arithmetic (mpmath 1.3.0) on the samples and theta of the three 50-digit fixtures that already exist
(mp_rbfbrownian_n134, matern_mp_m32_n134, matern_mp_m52_n134).

    Ky = K + (sigma_n^2 + 1e-8) I (none of the three needs jitter), Kinv = Ky^-1 by LU with partial pivoting, alpha = Kinv y,
    kd = diag Kinv,  c = 1/2 (1 / kd + alpha^2 / kd^2),  beta = Kinv (alpha / kd),
    G = -Kinv diag(c) Kinv + 1/2 (beta alpha^T + alpha beta^T),  d nlpd / d theta_p = -sum_ij G_ij dK_ij / dtheta_p

The kernels and their derivatives are written from their definitions here, as in gen_loo_golden.py; nothing of the engine or of
tests/loo_grad_oracle.py is used, which is what tests/test_oracle_loo_grad.py compares with these files.

    python tests/golden/gen_loo_grad_golden.py"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = (("mp_rbfbrownian_n134", "loo_grad_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_grad_mp_m32_n134"),
         ("matern_mp_m52_n134", "loo_grad_mp_m52_n134"))


def mp_loo_grad(kid, theta, X, y):
    import mpmath as mp
    mp.mp.dps = 50
    N = len(y)
    x = [mp.mpf(float(v)) for v in X[:, 0]]
    yv = mp.matrix([mp.mpf(float(v)) for v in y])
    th = [mp.mpf(repr(float(v))) for v in theta]
    sn = th[-1]

    def k_dk(a, b):
        """k(a, b) and its derivatives with respect to every kernel parameter (the noise excluded)."""
        if kid == 2:   # GPy RBF.K * Brownian.K for positive inputs: theta = (sigma_rbf^2, ell, sigma_b^2, sigma_n^2)
            k = th[0] * mp.e ** (-(a - b) ** 2 / (2 * th[1] ** 2)) * th[2] * min(a, b)
            return k, [k / th[0], k * (a - b) ** 2 / th[1] ** 3, k / th[2]]
        r = abs(a - b) / th[1]   # Matern, d = 1: theta = (sigma_f^2, ell, sigma_n^2)
        if kid == 3:
            s = mp.sqrt(3) * r
            return th[0] * (1 + s) * mp.e ** (-s), [(1 + s) * mp.e ** (-s), th[0] * s * s * mp.e ** (-s) / th[1]]
        s = mp.sqrt(5) * r
        return (th[0] * (1 + s + mp.mpf(5) / 3 * r * r) * mp.e ** (-s),
                [(1 + s + mp.mpf(5) / 3 * r * r) * mp.e ** (-s), th[0] * s * s * (1 + s) * mp.e ** (-s) / (3 * th[1])])

    nk = len(th) - 1
    Ky = mp.matrix(N, N)
    dK = [mp.matrix(N, N) for _ in range(nk)]
    for i in range(N):
        for j in range(N):
            Ky[i, j], dk = k_dk(x[i], x[j])
            for p in range(nk):
                dK[p][i, j] = dk[p]
        Ky[i, i] += sn + mp.mpf("1e-8")
    Kinv = mp.inverse(Ky)
    alpha = Kinv * yv
    kd = [Kinv[i, i] for i in range(N)]
    lpd = [-mp.log(2 * mp.pi / kd[i]) / 2 - alpha[i] ** 2 / (2 * kd[i]) for i in range(N)]
    c = [(1 / kd[i] + alpha[i] ** 2 / kd[i] ** 2) / 2 for i in range(N)]
    beta = Kinv * mp.matrix([alpha[i] / kd[i] for i in range(N)])
    KC = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            KC[i, j] = Kinv[i, j] * c[j]
    G = -(KC * Kinv)
    for i in range(N):
        for j in range(N):
            G[i, j] += (beta[i] * alpha[j] + alpha[i] * beta[j]) / 2
    grad = [-sum(G[i, j] * dK[p][i, j] for i in range(N) for j in range(N)) for p in range(nk)]
    grad.append(-sum(G[i, i] for i in range(N)))
    return -float(sum(lpd)), np.array([float(g) for g in grad])


def main():
    for src, dst in CASES:
        with np.load(os.path.join(OUT, src + ".npz"), allow_pickle=False) as z:
            kid, theta, X, y = int(z["kernel_id"]), z["theta"], z["X"], z["y"]
        assert X.shape[1] == 1 and kid in (2, 3, 4) and (kid != 2 or np.all(X > 0))
        nlpd, grad = mp_loo_grad(kid, theta, X, y)
        np.savez_compressed(os.path.join(OUT, dst + ".npz"), source="mpmath", fixture=src, kernel_id=kid, theta=theta,
                            nlpd=nlpd, grad=grad)
        print(dst, "nlpd", nlpd, "grad", grad)


if __name__ == "__main__":
    main()
