#!/usr/bin/env python3
"""Randomised sweep of the sliding windows' predictive gradients (cgp_window_predict_gradients: k_window_diag_inv,
k_window_alpha, k_window_pgrad behind the push kernels) against tests/window_pgrad_oracle.py (test infrastructure: uses
oracle/): random kernel (all five), window length N around the 16-sample blocks, input dimension, up to six windows with
hyper-parameters of their own, a number of ticks from {0, 1, N - 1, N, N + 1, 2 N + 3, 3 N + 6} (empty, filling, full, slid,
compacted, turned over twice), M around the 32-point chunk.  RBF x Brownian draws its test points after the window on the ticks
and inside it on and off the ticks.  The windows have no jitter ladder: a drawn case is skipped only when the oracle's fit of
some window needed jitter or raised NotPositiveDefinite; the last line says how many were, and more than 5 % of the drawn cases
skipped is a failure.
   python tests/fuzz/fuzz_window_pgrad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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
import pgrad_oracle as po
import window_pgrad_oracle as wo

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 100, 129, 200]
MS = [1, 15, 16, 17, 31, 32, 33, 100, 300]
TOL = 1e-6
t_end, cases, bad, skipped, worst = time.time() + budget, 0, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases + skipped < max_cases):
    N = int(rng.choice(NS))
    M = int(rng.choice(MS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 9))
    W = int(rng.integers(1, 7))
    T = int(rng.choice([0, 1, N - 1, N, N + 1, 2 * N + 3, 3 * N + 6]))
    seed = int(rng.integers(0, 1 << 30))
    cap = max(N, 2)   # cgp_window_init takes N >= 2: a window of one sample is a capacity-2 window after one tick
    if N == 1:
        T = min(T, 1)
    Xw, yw, Xsw = [], [], []
    for w in range(W):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + max(T, 1), dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=len(t)) for _ in range(d - 1)])
        lo = max(len(t) - cap, 0)   # first sample still in the window
        if kid == 2:
            after = t[-1] + 1.0 + np.arange(M, dtype=np.float64)
            tick = t[r2.integers(lo, len(t), size=M)]
            inside = np.where(r2.random(M) < 0.5, tick, tick + r2.uniform(0.1, 0.9, size=M))
            Xs = np.where(r2.random(M) < 0.5, after, inside)[:, None]
        else:
            Xs = X[r2.integers(lo, len(t), size=M)] + 0.3 * r2.normal(size=(M, d))
        Xw.append(X[:T]); yw.append(y[:T]); Xsw.append(Xs)
    X, y, Xs = np.stack(Xw), np.stack(yw), np.stack(Xsw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (W, 1)) * (0.7 + 0.6 * rng.random((W, 1)))   # every parameter of a window scaled by the window's own factor
    tag = f"N={N} M={M} d={d} kid={kid} W={W} T={T} seed={seed}"
    try:
        fits = [wo.window_fit(kid, theta[w], cap, X[w], y[w]) for w in range(W)]
        if any(f is not None and f.jitter != 0.0 for f in fits):
            raise po.go.NotPositiveDefinite("jitter")
        ref = [wo.sliding_window_gradients(kid, theta[w], cap, X[w], y[w], Xs[w]) for w in range(W)]
    except po.go.NotPositiveDefinite:
        skipped += 1
        print("skipped (the oracle's fit of a window needs jitter)", tag)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, cap, d, kid, theta)
    if T:
        ctx.window_push(X, y)
    mean, var, dmean, dvar = ctx.window_predict_gradients(Xs)
    for w, (odm, odv) in enumerate(ref):
        if T == 0:   # the prior rule holds exactly
            ok, e = bool(np.all(dmean[w] == 0.0) and np.array_equal(dvar[w], odv)), 0.0
        else:
            em = np.max(np.abs(dmean[w] - odm)) / max(np.max(np.abs(odm)), 1e-300)
            ev = np.max(np.abs(dvar[w] - odv)) / max(np.max(np.abs(odv)), 1e-300)
            e = max(em, ev)
            ok = e <= TOL
        worst = max(worst, e / TOL) if ok else worst
        if not ok:
            print("FAIL", tag, "window", w, "dmean", dmean[w].ravel()[:4], odm.ravel()[:4], "dvar", dvar[w].ravel()[:4], odv.ravel()[:4]); bad += 1
    ctx.close()
too_many = skipped > 0.05 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 5 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
