#!/usr/bin/env python3
"""Randomised sweep of the sliding-window engine (k_window_ticks, k_window_pairs, k_window_multi) against the refit-per-tick oracle
(test infrastructure: uses oracle/ and tests/matern_oracle.py): random window length N (around the 16-column panel boundaries, and
long ones either side of the LDS limits of the four-tick and the packed kernels), input dimension up to 8, the five kernels,
stream length (several ring compactions), number of independent windows (either side of the kernels' crossovers) and block cuts.
   python tests/fuzz/fuzz_window.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
from corenav_gp_amd import engine, synth
from oracle import gp_oracle as go
import matern_oracle as mo

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
NS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100, 129, 200, 333, 512, 543, 544, 545, 546, 547, 700]
MANY = [256, 257, 512, 1024]   # either side of the single-tick kernel's thread counts, four ticks per pass, two windows per workgroup
FACTOR_BYTES = 10e9            # of a case's factors, nwin (2 N)^2 doubles
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0
nmany = nlong = nmat = 0   # cases of >= 256 windows, of N >= 200, of a Matern kernel
while time.time() < t_end:
    N = int(rng.choice(NS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == synth.KERNEL_RBF_BROWNIAN else int(rng.integers(1, 9))
    T = int(rng.integers(max(2, N // 2), 3 * N + 20))
    nwin = int(rng.integers(1, 4))
    if N >= 32 and rng.integers(0, 3) == 0:   # many windows: three of them are compared
        nwin = int(rng.choice([v for v in MANY if v * (2.0 * N) ** 2 * 8 <= FACTOR_BYTES]))
    noise = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1 << 30))
    Xs, ys = [], []
    for w in range(nwin):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + T, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / t.std()] + [r2.normal(size=T) for _ in range(d - 1)])
        Xs.append(X); ys.append(y)
    X, y = np.stack(Xs), np.stack(ys)
    ard = np.concatenate([[0.02], np.linspace(0.8, 1.6, d) * np.sqrt(d), [1e-3]])
    theta = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, np.sqrt(d), 1e-3]), 1: ard, 3: ard, 4: ard}[kid]
    om = mo if kid >= 3 else go
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, theta)
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(1, T, size=int(rng.integers(0, 4)))]))
    outs = [ctx.window_push(X[:, a:b], y[:, a:b], include_noise=noise) for a, b in zip(cuts[:-1], cuts[1:])]
    pm, pv, lm = [np.concatenate([o[i] for o in outs], axis=1) for i in range(3)]
    cases += 1
    nmany, nlong, nmat = nmany + (nwin >= 256), nlong + (N >= 200), nmat + (kid >= 3)
    tag = f"N={N} d={d} kid={kid} T={T} nwin={nwin} noise={noise} cuts={cuts} seed={seed}"
    for w in (range(nwin) if nwin <= 4 else sorted({0, nwin - 1, int(rng.integers(0, nwin))})):
        kdiag = om.kernel_Kdiag(kid, theta, X[w])
        if N < 200:
            ticks = np.arange(T)
            opm, opv, olm = om.sliding_window_stream(kid, theta, N, X[w], y[w], include_noise=noise)
        else:
            # a long window: refits at a handful of ticks keep the oracle's share of a case to about a second -- the first steady
            # ticks, either side of the block cuts and of the first ring compaction, the last tick
            ticks = np.array(sorted({t for t in [1, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, T - 1] + [c - 1 for c in cuts[1:-1]] + cuts[1:-1]
                                     if 0 < t < T})[:12])
            opm, opv, olm = np.empty(len(ticks)), np.empty(len(ticks)), np.empty(len(ticks))
            for i, t in enumerate(ticks):
                lo = max(0, t - N + 1)
                mu, var = om.predict(om.fit(kid, theta, X[w][lo:t], y[w][lo:t]), X[w][t:t + 1], noise)
                opm[i], opv[i], olm[i] = mu[0], var[0], om.fit(kid, theta, X[w][max(0, t + 1 - N):t + 1], y[w][max(0, t + 1 - N):t + 1]).logml
        scale = np.abs(opv) if noise else np.maximum(np.abs(opv), 1e-9 * kdiag[ticks])
        e = max(float(np.max(np.abs(pm[w][ticks] - opm)) / max(np.max(np.abs(opm)), 1e-12 if N < 200 else 1e-3)),
                float(np.max(np.abs(pv[w][ticks] - opv) / scale)), float(np.max(np.abs(lm[w][ticks] - olm) / np.maximum(np.abs(olm), 1.0))))
        worst = max(worst, e / 1e-6)
        if not (e < 1e-6) or ctx.window_state(w) != (min(N, T), 0):
            print("FAIL", tag, "window", w, "err", e, "state", ctx.window_state(w)); bad += 1
print(f"cases {cases} failures {bad} worst error / bar {worst:.3g} (of them {nmany} of >= 256 windows, {nlong} of N >= 200, {nmat} Matern)")
sys.exit(1 if bad else 0)
