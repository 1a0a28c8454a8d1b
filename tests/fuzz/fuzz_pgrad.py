#!/usr/bin/env python3
"""Randomised sweep of the predictive gradients after batch fits (cgp_fit_predict_grad_batch: the tiled fit schedules,
k_pgrad_solve, k_pgrad_contract) against tests/pgrad_oracle.py (test infrastructure: uses oracle/): random kernel (all five),
window length N <= 400 (around the 16-sample blocks and the 128-column tiles of the panel), M <= 300 (around the 64 test points
of a contraction workgroup and the 128-row tiles of the solve), input dimension and batch <= 40 (latency and mid-size
schedules).  RBF x Brownian draws its test points after the window on the ticks and inside it on and off the ticks.  A drawn
case is skipped only when the oracle's own jitter ladder rejects it (NotPositiveDefinite); the last line says how many were, and
more than 5 % of the drawn cases skipped is a failure.
   python tests/fuzz/fuzz_pgrad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 134, 161, 191, 192, 193, 200, 255, 256, 257, 301, 385, 400]
MS = [1, 2, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 130, 255, 256, 300]
BS = [1, 2, 3, 5, 17, 30, 40]
TOL = 1e-6
t_end, cases, bad, skipped, worst = time.time() + budget, 0, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases + skipped < max_cases):
    N = int(rng.choice(NS))
    M = int(rng.choice(MS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 9))
    B = int(rng.choice(BS))
    seed = int(rng.integers(0, 1 << 30))
    Xw, yw, Xsw = [], [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=N) for _ in range(d - 1)])
        if kid == 2:
            after = t[-1] + 1.0 + np.arange(M, dtype=np.float64)
            inside = np.where(r2.random(M) < 0.5, t[r2.integers(0, N, size=M)], t[r2.integers(0, N, size=M)] + r2.uniform(0.1, 0.9, size=M))
            Xs = np.where(r2.random(M) < 0.5, after, inside)[:, None]
        else:
            Xs = X[r2.integers(0, N, size=M)] + 0.3 * r2.normal(size=(M, d))
        Xw.append(X); yw.append(y); Xsw.append(Xs)
    X, y, Xs = np.stack(Xw), np.stack(yw), np.stack(Xsw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (B, 1)) * (0.7 + 0.6 * rng.random((B, 1)))   # every parameter of a fit scaled by the fit's own factor
    tag = f"N={N} M={M} d={d} kid={kid} B={B} seed={seed}"
    check = list(range(B)) if B <= 3 else sorted({0, B - 1, int(rng.integers(0, B))})
    try:
        ref = [po.predictive_gradients(po.fit(kid, theta[b], X[b], y[b]), Xs[b]) for b in check]
    except po.go.NotPositiveDefinite:
        skipped += 1
        print("skipped (the oracle's jitter ladder rejects it)", tag)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    assert ctx.pgrad_reserve(B, M) == 0
    rc, mean, var, logml, info, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid)
    for b, (odm, odv) in zip(check, ref):
        em = np.max(np.abs(dmean[b] - odm)) / max(np.max(np.abs(odm)), 1e-300)
        ev = np.max(np.abs(dvar[b] - odv)) / max(np.max(np.abs(odv)), 1e-300)
        e = max(em, ev)
        ok = info[b] == 0 and e <= TOL
        worst = max(worst, e / TOL) if ok else worst
        if not ok:
            print("FAIL", tag, "fit", b, "dmean", em, "dvar", ev, "info", info[b]); bad += 1
    ctx.close()
too_many = skipped > 0.05 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 5 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
