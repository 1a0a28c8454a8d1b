#!/usr/bin/env python3
"""Randomised sweep of the multi-target sliding windows (cgp_window_push_multi / cgp_window_predict_multi:
k_window_targets_store in front of the push kernels, k_window_diag_inv, the Z solve and the forecast's mean epilogue) against
tests/window_multi_oracle.py (test infrastructure: uses oracle/): random kernel (all five), window length N around the
16-sample blocks, input dimension, up to six windows with hyper-parameters of their own, P around the 16-column target tile, a
number of ticks from {0, 1, N - 1, N, N + 1, 2 N + 3, 3 N + 6} fed in one, two or three pushes, M around the 32-point chunk.  Also
checked per case: var is bitwise cgp_window_predict's.  The windows have no jitter ladder: a drawn case is skipped only when the
oracle's fit of some window needed jitter or raised NotPositiveDefinite; the last line says how many were, and more than 5 % of
the drawn cases skipped is a failure.
   python tests/fuzz/fuzz_window_multi.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
oracle-only: no GPU -- draws the same cases and runs the oracle alone (to see how many a seed's prefix skips)."""
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
import window_multi_oracle as wm

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [2, 15, 16, 17, 31, 33, 63, 64, 65, 100, 129, 200]
MS = [1, 15, 16, 17, 31, 32, 33, 100, 300]
PS = [1, 2, 3, 15, 16, 17, 33, 64]
TOL = 1e-6
t_end, cases, bad, skipped, worst = time.time() + budget, 0, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases + skipped < max_cases):
    N = int(rng.choice(NS))
    M = int(rng.choice(MS))
    P = int(rng.choice(PS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 9))
    W = int(rng.integers(1, 7))
    T = int(rng.choice([0, 1, N - 1, N, N + 1, 2 * N + 3, 3 * N + 6]))
    cuts = sorted(set(int(c) for c in rng.integers(0, T + 1, size=2)) | {T})
    seed = int(rng.integers(0, 1 << 30))
    Xw, Yw, Xsw = [], [], []
    for w in range(W):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + max(T, 1), dtype=np.float64)
        Y = np.column_stack([(1.0 + 0.25 * p) * synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1) + w), t) for p in range(P)])
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=len(t)) for _ in range(d - 1)])
        lo = max(len(t) - N, 0)   # first sample still in the window
        if kid == 2:
            after = t[-1] + 1.0 + np.arange(M, dtype=np.float64)
            tick = t[r2.integers(lo, len(t), size=M)]
            inside = np.where(r2.random(M) < 0.5, tick, tick + r2.uniform(0.1, 0.9, size=M))
            Xs = np.where(r2.random(M) < 0.5, after, inside)[:, None]
        else:
            Xs = X[r2.integers(lo, len(t), size=M)] + 0.3 * r2.normal(size=(M, d))
        Xw.append(X[:T]); Yw.append(Y[:T]); Xsw.append(Xs)
    X, Y, Xs = np.stack(Xw), np.stack(Yw), np.stack(Xsw)
    th1 = wm.theta_of(kid, d)
    theta = np.tile(th1, (W, 1)) * (0.7 + 0.6 * rng.random((W, 1)))   # every parameter of a window scaled by the window's own factor
    noise = bool(rng.integers(0, 2))
    tag = f"N={N} M={M} P={P} d={d} kid={kid} W={W} T={T} cuts={cuts} seed={seed}"
    try:
        ref = [wm.sliding_window_forecast_multi(kid, theta[w], N, X[w], Y[w], Xs[w], noise, want_jitter=True) for w in range(W)]
        if any(r[3] != 0.0 for r in ref):
            raise go.NotPositiveDefinite("jitter")
    except go.NotPositiveDefinite:
        skipped += 1
        print("skipped (the oracle's fit of a window needs jitter)", tag)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    ctx.window_multi_reserve(P)
    fed = 0
    for c in cuts:
        if c > fed:
            ctx.window_push_multi(X[:, fed:c], Y[:, fed:c])
            fed = c
    mean, var, logml = ctx.window_predict_multi(Xs, include_noise=noise)
    _, v0 = ctx.window_predict(Xs, include_noise=noise)
    if not np.array_equal(var, v0):
        print("FAIL", tag, "var is not bitwise cgp_window_predict's"); bad += 1
    for w, (om, ov, ol, _) in enumerate(ref):
        if T == 0:   # the prior rule holds exactly
            ok, e = bool(np.all(mean[w] == 0.0) and np.all(logml[w] == 0.0) and np.allclose(var[w], ov, rtol=1e-14, atol=0.0)), 0.0
        else:
            e = max(wm.errors(mean[w], var[w], logml[w], om, ov, ol))
            ok = e <= TOL
        worst = max(worst, e / TOL) if ok else worst
        if not ok:
            print("FAIL", tag, "window", w, "mean", mean[w].ravel()[:4], om.ravel()[:4], "var", var[w][:4], ov[:4], "logml", logml[w][:4], ol[:4]); bad += 1
    ctx.close()
too_many = skipped > 0.05 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 5 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
