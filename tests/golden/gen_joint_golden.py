#!/usr/bin/env python3
"""Writes closed_joint_n2_se.npz: the joint forecast (mean, full posterior covariance, two sample paths) of a window of TWO
samples under the SE-iso kernel, from formulas written out here (the 2 x 2 inverse by hand; nothing of oracle/).  The C caller of
the joint forecast (tests/c_abi/window_joint.c) and tests/test_oracle_window_joint.py check against it.
   python tests/golden/gen_joint_golden.py"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    sf2, ell, sn2 = 0.8, 1.5, 0.01
    theta = np.array([sf2, ell, sn2])
    X = np.array([[0.0], [1.0]])
    y = np.array([0.3, -0.2])
    Xs = np.array([[-1.0], [0.25], [0.5], [2.0], [3.5]])
    k = lambda a, b: sf2 * np.exp(-0.5 * (a - b) ** 2 / ell ** 2)
    a, b = k(0.0, 0.0) + sn2 + 1e-8, k(0.0, 1.0)          # Ky = [[a, b], [b, a]] (the engine's fixed 1e-8 jitter included)
    det = a * a - b * b
    Kinv = np.array([[a, -b], [-b, a]]) / det
    Ks = np.array([[k(x[0], s[0]) for s in Xs] for x in X])   # (2, M)
    mean = Ks.T @ (Kinv @ y)
    cov = np.array([[k(s[0], t[0]) for t in Xs] for s in Xs]) - Ks.T @ Kinv @ Ks
    cov = 0.5 * (cov + cov.T)
    M = len(Xs)
    jitter_rel = 1e-6
    A = cov + sn2 * np.eye(M)                              # include_noise = 1
    A = A + jitter_rel * np.mean(np.diag(A)) * np.eye(M)
    C = np.linalg.cholesky(A)
    xi = np.array([[0.5, -1.0, 0.25, 2.0, -0.75], [1.0, 0.0, -0.5, 0.125, 1.5]])
    paths = mean[None, :] + xi @ C.T
    np.savez_compressed(os.path.join(OUT, "closed_joint_n2_se.npz"), source="closed", kernel_id=0, theta=theta, X=X, y=y, Xs=Xs,
                        mean=mean, cov_latent=cov, noise=sn2, jitter_rel=jitter_rel, xi=xi, paths=paths)


if __name__ == "__main__":
    main()
