#!/usr/bin/env python3
"""Randomised sweep of the sliding windows' joint forecast (cgp_window_predict_cov / cgp_window_sample: the solve with V kept,
k_window_joint_cov, k_window_joint_chol, k_window_joint_paths) against the refit oracle (test infrastructure: uses oracle/):
random kernel, window length N (around the 16-row block boundaries and the forms of the solve), input dimension, number of
windows, push pattern, number of test points M (around the 16- and 64-point tile boundaries) and of paths S; joint forecasts at
random moments of the stream -- empty, filling, full, either side of a ring compaction.
   python tests/fuzz/fuzz_window_joint.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
from corenav_gp_amd import engine, synth
from oracle import gp_oracle as go
from joint_oracle import sliding_window_joint, sample_paths

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
NS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100, 129, 200]
MS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 300]
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0
while time.time() < t_end:
    N = int(rng.choice(NS))
    if rng.integers(0, 40) == 0:
        N = int(rng.choice([513, 600, 1025, 1100]))     # the one-tile and the half-tile form of the solve
    kid = int(rng.integers(0, 3))
    d = 1 if kid == synth.KERNEL_RBF_BROWNIAN else int(rng.integers(1, 7))
    T = int(rng.integers(2, 3 * N + 20)) if N <= 200 else int(rng.integers(N // 2, N + 40))
    nwin = int(rng.integers(1, 4))
    if N <= 64 and rng.integers(0, 6) == 0:
        nwin = int(rng.integers(100, 400))
    seed = int(rng.integers(0, 1 << 30))
    Xw, yw = [], []
    for w in range(nwin):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + T, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / t.std()] + [r2.normal(size=T) for _ in range(d - 1)])
        Xw.append(X); yw.append(y)
    X, y = np.stack(Xw), np.stack(yw)
    theta = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]),
             1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]
    max_m = int(rng.choice([300, 304, 599])) if nwin <= 4 else 128
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, theta)
    ctx.window_joint_reserve(max_m)
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(0, T + 1, size=int(rng.integers(0, 3)))]))
    for a, b in zip([0] + cuts[:-1], cuts):           # a forecast before the first push (empty windows) and after every block
        if b > a:
            ctx.window_push(X[:, a:b], y[:, a:b])
        M = min(int(rng.choice(MS)), max_m)
        S = int(rng.choice([1, 3, 16, 17, 40]))
        noise = bool(rng.integers(0, 2))
        if kid == 2:
            Xs = X[:, max(b, 1) - 1:max(b, 1), :] + 1.0 + np.arange(M, dtype=np.float64)[None, :, None] + np.zeros((nwin, 1, 1))
        else:
            Xs = X[:, rng.integers(max(0, b - N), max(b, 1), size=M)] + 0.3 * rng.normal(size=(nwin, M, d))
        xi = rng.normal(size=(nwin, S, M))
        mean, cov = ctx.window_predict_cov(Xs, include_noise=noise)
        pm, pv = ctx.window_predict(Xs, include_noise=noise)
        paths, info = ctx.window_sample(Xs, xi, include_noise=True, jitter_rel=1e-6)   # with noise: a well-conditioned factor
        cases += 1
        tag = f"N={N} d={d} kid={kid} T={T} nwin={nwin} at={b} M={M} S={S} noise={noise} cuts={cuts} seed={seed}"
        for w in (range(nwin) if nwin <= 4 else sorted({0, nwin - 1, int(rng.integers(0, nwin))})):
            omu, ocov = sliding_window_joint(kid, theta, N, X[w, :b], y[w, :b], Xs[w], include_noise=noise)
            sd = np.sqrt(np.maximum(np.diag(ocov), 1e-9 * go.kernel_Kdiag(kid, theta, Xs[w]) + 1e-300))
            e = max(float(np.max(np.abs(mean[w] - omu)) / max(np.max(np.abs(omu)), 1e-12)), float(np.max(np.abs(cov[w] - ocov) / np.outer(sd, sd))))
            lat = ocov - (go.noise_var(kid, theta) if noise else 0.0) * np.eye(M)
            op = sample_paths(omu, lat, go.noise_var(kid, theta), 1e-6, xi[w])
            e = max(e, float(np.max(np.abs(paths[w] - op)) / max(np.max(np.abs(op)), 1e-12)))
            worst = max(worst, e / 1e-6)
            exact = np.array_equal(cov[w], cov[w].T) and np.array_equal(mean[w], pm[w]) and np.array_equal(np.diag(cov[w]), pv[w])
            if not (e < 1e-6) or not exact or info[w] != 0 or ctx.window_state(w) != (min(N, b), 0):
                print("FAIL", tag, "window", w, "err", e, "exact", exact, "info", info[w], "state", ctx.window_state(w)); bad += 1
    ctx.close()
print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
sys.exit(1 if bad else 0)
