#!/usr/bin/env python3
"""Randomised sweep of the joint forecast after batch fits (cgp_fit_predict_cov_batch / cgp_fit_sample_batch: the tiled fit
schedules, k_joint_cov, k_window_joint_chol, k_window_joint_paths) against the refit oracle (test infrastructure: uses oracle/):
random kernel (all five), window length N (around the 4-, 16- and 128-column boundaries of the contraction and the panel),
input dimension, batch (latency, mid-size and fused schedules), number of test points M (around the 16- and 64-point tile
boundaries and the 128-row tile of the extra rows) and of paths S.  A drawn case is dropped only when the oracle itself raises
LinAlgError on it; the last line says how many were.
   python tests/fuzz/fuzz_joint_batch.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
oracle-only: no GPU -- draws the same cases and runs the oracle alone (to see which prefix of a seed drops nothing)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
oracle_only = "oracle-only" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "oracle-only"]
if not oracle_only:
    import torch  # noqa: F401
    from corenav_gp_amd import engine
from corenav_gp_amd import synth
from oracle import gp_oracle as go
from joint_oracle import sliding_window_joint, sample_paths
import matern_oracle as mo

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129, 134, 161, 200, 255, 257, 301, 385]
MS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 126, 127, 128, 129, 300]
BS = [1, 2, 3, 5, 30, 50, 70]
t_end, cases, bad, dropped, worst = time.time() + budget, 0, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases + dropped < max_cases):
    N = int(rng.choice(NS))
    if rng.integers(0, 30) == 0:
        N = int(rng.choice([513, 700, 1025]))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 7))
    B = int(rng.choice(BS)) if N <= 400 else int(rng.integers(1, 4))
    M = int(rng.choice(MS))
    S = int(rng.choice([1, 3, 16, 17, 40]))
    noise = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1 << 30))
    Xw, yw, Xsw = [], [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / t.std()] + [r2.normal(size=N) for _ in range(d - 1)])
        Xs = X[-1:, :] + 1.0 + np.arange(M, dtype=np.float64)[:, None] if kid == 2 else \
            X[r2.integers(max(0, N - 50), N, size=M)] + 0.3 * r2.normal(size=(M, d))
        Xw.append(X); yw.append(y); Xsw.append(Xs)
    X, y, Xs = np.stack(Xw), np.stack(yw), np.stack(Xsw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (B, 1))
    xi = np.random.default_rng(seed + 99).normal(size=(B, S, M))
    sn = float(th1[-1]) if kid >= 3 else go.noise_var(kid, th1)
    tag = f"N={N} d={d} kid={kid} B={B} M={M} S={S} noise={noise} seed={seed}"
    check = list(range(B)) if B <= 3 else sorted({0, B - 1, int(rng.integers(0, B))})
    try:
        ref = []
        for b in check:
            if kid >= 3:
                omu, ocov = mo.predict_cov(mo.fit(kid, theta[b], X[b], y[b]), Xs[b], noise)
            else:
                omu, ocov = sliding_window_joint(kid, theta[b], N, X[b], y[b], Xs[b], include_noise=noise)
            lat = ocov - (sn if noise else 0.0) * np.eye(M)
            ref.append((omu, ocov, sample_paths(omu, lat, sn, 1e-6, xi[b])))   # with noise: a well-conditioned factor
    except np.linalg.LinAlgError:
        dropped += 1
        print("dropped (the oracle raised LinAlgError)", tag)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    ctx.joint_reserve(B, M)
    rc, mean, cov, logml, info = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=noise)
    rc2, paths, _, _, sinfo = ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=True, jitter_rel=1e-6)
    for b, (omu, ocov, op) in zip(check, ref):
        kd = th1[0] * (np.abs(Xs[b][:, 0]) * th1[2] if kid == 2 else np.ones(M))
        sd = np.sqrt(np.maximum(np.diag(ocov), 1e-9 * kd + 1e-300))
        e = max(float(np.max(np.abs(mean[b] - omu)) / max(np.max(np.abs(omu)), 1e-12)), float(np.max(np.abs(cov[b] - ocov) / np.outer(sd, sd))))
        e = max(e, float(np.max(np.abs(paths[b] - op)) / max(np.max(np.abs(op)), 1e-12)))
        worst = max(worst, e / 1e-6)
        exact = np.array_equal(cov[b], cov[b].T)
        if not (e < 1e-6) or not exact or info[b] != 0 or sinfo[b] != 0:
            print("FAIL", tag, "fit", b, "err", e, "symmetric", exact, "info", info[b], "sinfo", sinfo[b]); bad += 1
    ctx.close()
print(f"cases {cases} failures {bad} dropped {dropped} worst error / bar {worst:.3g}")
sys.exit(1 if bad else 0)
