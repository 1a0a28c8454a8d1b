#!/usr/bin/env python3
"""Randomised sweep of the multi-target windows' summed objective (cgp_window_multi_nll_grad: k_window_diag_inv, the Z solve,
k_window_multi_alpha, the contraction with the rank-P term, the finish) against tests/window_multi_opt_oracle.py (test
infrastructure: uses oracle/), with the generator of tests/fuzz/fuzz_window_multi.py, draw for draw: random kernel (all five),
window length N around the 16-sample blocks, input dimension, up to six windows with hyper-parameters of their own, P around the
16-column target tile, a number of ticks from {0, 1, N - 1, N, N + 1, 2 N + 3, 3 N + 6} fed in one, two or three pushes.  Also
checked per case: logml is bitwise cgp_window_predict_multi's, and logml = NULL leaves nll and the gradient identical.  The windows
have no jitter ladder: a drawn case is skipped only when the oracle's fit of some window needed jitter or raised
NotPositiveDefinite; the last line says how many were, and more than 5 % of the drawn cases skipped is a failure.
   python tests/fuzz/fuzz_window_multi_opt.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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
import window_multi_opt_oracle as wmo

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
    M = int(rng.choice(MS))   # (the forecast sweep's draw: kept so that a seed names the same windows in both sweeps)
    P = int(rng.choice(PS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 9))
    W = int(rng.integers(1, 7))
    T = int(rng.choice([0, 1, N - 1, N, N + 1, 2 * N + 3, 3 * N + 6]))
    cuts = sorted(set(int(c) for c in rng.integers(0, T + 1, size=2)) | {T})
    seed = int(rng.integers(0, 1 << 30))
    Xw, Yw = [], []
    for w in range(W):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + max(T, 1), dtype=np.float64)
        Y = np.column_stack([(1.0 + 0.25 * p) * synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1) + w), t) for p in range(P)])
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=len(t)) for _ in range(d - 1)])
        Xw.append(X[:T]); Yw.append(Y[:T])
    X, Y = np.stack(Xw).reshape(W, T, d), np.stack(Yw).reshape(W, T, P)
    th1 = wm.theta_of(kid, d)
    theta = np.tile(th1, (W, 1)) * (0.7 + 0.6 * rng.random((W, 1)))   # every parameter of a window scaled by the window's own factor
    rng.integers(0, 2)   # (the forecast sweep's include_noise draw)
    tag = f"N={N} P={P} d={d} kid={kid} W={W} T={T} cuts={cuts} seed={seed}"
    try:
        if T > 0 and any(wmo.jitter(kid, theta[w], N, X[w], Y[w]) != 0.0 for w in range(W)):
            raise go.NotPositiveDefinite("jitter")
        ref = [wmo.nll_and_grad_multi(kid, theta[w], N, X[w], Y[w], T) for w in range(W)]
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
    ctx.window_multi_grad_reserve()
    fed = 0
    for c in cuts:
        if c > fed:
            ctx.window_push_multi(X[:, fed:c], Y[:, fed:c])
            fed = c
    nll, g, logml = ctx.window_multi_nll_grad()
    nll2, g2, _ = ctx.window_multi_nll_grad(want_logml=False)
    _, _, l0 = ctx.window_predict_multi(np.ones((W, 1, d)))
    if not (np.array_equal(nll, nll2) and np.array_equal(g, g2) and np.array_equal(logml, l0)):
        print("FAIL", tag, "logml = NULL moved nll / grad, or logml is not bitwise cgp_window_predict_multi's"); bad += 1
    for w, (onll, og, ol) in enumerate(ref):
        if T == 0:   # the empty-window rule holds exactly
            ok, e = bool(nll[w] == 0.0 and np.all(g[w] == 0.0) and np.all(logml[w] == 0.0)), 0.0
        else:
            e = max(abs(nll[w] - onll) / max(abs(onll), 1.0), np.max(np.abs(g[w] - og)) / np.max(np.abs(og)),
                    np.max(np.abs(logml[w] - ol) / np.maximum(1.0, np.abs(ol))))
            ok = e <= TOL
        worst = max(worst, e / TOL) if ok else worst
        if not ok:
            print("FAIL", tag, "window", w, "nll", nll[w], onll, "grad", g[w], og, "logml", logml[w][:4], ol[:4]); bad += 1
    ctx.close()
too_many = skipped > 0.05 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 5 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
