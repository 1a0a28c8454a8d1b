#!/usr/bin/env python3
"""Randomised sweep of the Matern kernels through cgp_fit_predict_batch and cgp_nll_grad against tests/matern_oracle.py (test
infrastructure): random kernel of the two, N 2 ... 700, d 1 ... 6, M 1 ... 700, batch 1 ... 96, theta log-uniform, dense grids (unit-spaced
ticks, d = 1) and sparse ones (random points).  One bar: 1e-6 on mean, variance
and logML, the gradient to 1e-6 of its largest entry, and the jitter ladder's outcome (info, jitter added) equal to the oracle's.
   python tests/fuzz/fuzz_matern.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
from corenav_gp_amd import engine
import matern_oracle as mo

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
TOL = 1e-6
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0
while time.time() < t_end:
    kid = int(rng.choice(mo.KERNELS))
    N = int(rng.choice([2, 3, 15, 16, 17, 127, 128, 129, 134, 160, 161, 255, 256, 257, 300, 511, 513, 700])) if rng.integers(0, 2) else int(rng.integers(2, 701))
    dense = bool(rng.integers(0, 3) == 0)
    d = 1 if dense else int(rng.integers(1, 7))
    M = int(rng.choice([1, 15, 16, 17, 127, 128, 129, 599, 700])) if rng.integers(0, 2) else int(rng.integers(1, 701))
    B = int(rng.choice([1, 2, 3, 24, 40, 56, 96])) if N <= 300 else int(rng.integers(1, 5))
    if dense:
        t0 = float(rng.integers(0, 500))
        X = np.tile((t0 + np.arange(N, dtype=np.float64))[None, :, None], (B, 1, 1))
        Xs = np.tile((t0 + N + np.arange(M, dtype=np.float64))[None, :, None], (B, 1, 1))
        ell = np.exp(rng.uniform(np.log(0.5), np.log(60.0), (B, 1)))
    else:
        X = rng.uniform(-2.0, 2.0, (B, N, d))
        Xs = rng.uniform(-2.5, 2.5, (B, M, d))
        ell = np.exp(rng.uniform(np.log(0.2), np.log(8.0), (B, d)))
    y = np.sin(X.sum(2) / (8.0 if dense else 1.0)) * rng.uniform(0.1, 2.0, (B, 1)) + 0.05 * rng.normal(size=(B, N))
    # dense grids: sigma_f^2 / sigma_n^2 <= 1e4 (the reference's window sits at 25).  The relative error of a posterior variance far
    # below the prior one grows with that ratio for ANY fp64 factorisation, the oracle's included: with ratios up to 1e6 one dense
    # N = 556 Matern 5/2 window in 1 086 cases came out at 1.75e-6
    sf2 = np.exp(rng.uniform(np.log(1e-2), np.log(1.0 if dense else 10.0), B))
    th = np.column_stack([sf2, ell, np.exp(rng.uniform(np.log(1e-4 if dense else 1e-5), np.log(0.1), B))])
    ctx = engine.Context(max_n=N, max_m=max(M, N), max_d=d, max_batch=B)
    rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th, kid)
    err, why = 0.0, ""
    for b in sorted({0, B // 2, B - 1}):
        try:
            f = mo.fit(kid, th[b], X[b], y[b])
        except np.linalg.LinAlgError:
            if info[b] == 0:
                err, why = 1.0, "the oracle's ladder failed, the engine's did not"
            continue
        if info[b] != 0:
            err, why = 1.0, f"info {info[b]} where the oracle succeeded (jitter {f.jitter})"
            continue
        omu, ovar = mo.predict(f, Xs[b])
        e = max(float(np.max(np.abs(mean[b] - omu)) / max(np.max(np.abs(omu)), 1e-300)), float(np.max(np.abs(var[b] - ovar) / ovar)),
                abs(logml[b] - f.logml) / max(abs(f.logml), 1.0))
        if f.jitter == 0.0 and b == 0:       # the gradient entry point on the same window (one ladder outcome: none needed)
            nll, g = ctx.nll_grad(X[b], y[b], kid, th[b])
            onll, og = mo.nll_and_grad(kid, th[b], X[b], y[b])
            e = max(e, abs(nll - onll) / max(abs(onll), 1.0), float(np.max(np.abs(g - og)) / np.max(np.abs(og))))
            if ctx.last_jitter() != 0.0:
                e, why = 1.0, "jitter added where the oracle needed none"
        err = max(err, e)
    ctx.close()
    cases += 1
    worst = max(worst, err)
    if not err < TOL:
        bad += 1
        print(f"FAIL kid {kid} N {N} d {d} M {M} B {B} dense {dense} err {err:.3e} theta[0] {th[0].tolist()} {why}", flush=True)
print(f"cases {cases} failures {bad} worst {worst:.3e}")
sys.exit(1 if bad else 0)
