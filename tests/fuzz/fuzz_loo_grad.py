#!/usr/bin/env python3
"""Randomised sweep of the leave-one-out objective (cgp_loo_nll_grad_batch: the tiled fit schedules in gradient mode, k_loo,
k_loo_kinv, k_loo_beta, k_loo_grad) against tests/loo_grad_oracle.py (test infrastructure: uses oracle/): random kernel (all
five), window length N <= 301 (around the 128-sample tiles: one, two and three block steps), input dimension and batch <= 40
(latency and mid-size schedules).  Bar: 1e-6, nlpd relative and the gradient against its largest component.  A drawn case is
skipped, and counted, when the oracle needs jitter (or its ladder rejects it) or when the oracle's closed form misses its own
central difference by more than 1e-8 of max|grad| on a checked fit: the bar then would measure the oracle.  More than 10 % of
the drawn cases skipped is a failure.
   python tests/fuzz/fuzz_loo_grad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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
import loo_oracle as lo
import loo_grad_oracle as lgo

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [1, 2, 3, 15, 17, 64, 100, 127, 128, 129, 134, 161, 200, 255, 256, 257, 301]
BS = [1, 2, 3, 5, 17, 30, 40]
TOL, SELF = 1e-6, 1e-8
t_end, cases, bad, skipped, worst = time.time() + budget, 0, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases + skipped < max_cases):
    N = int(rng.choice(NS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 7))
    B = int(rng.choice(BS))
    seed = int(rng.integers(0, 1 << 30))
    Xw, yw = [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=N) for _ in range(d - 1)])
        Xw.append(X); yw.append(y)
    X, y = np.stack(Xw), np.stack(yw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (B, 1)) * (0.7 + 0.6 * rng.random((B, 1)))   # every parameter of a fit scaled by the fit's own factor
    tag = f"N={N} d={d} kid={kid} B={B} seed={seed}"
    check = list(range(B)) if B <= 2 else sorted({0, B - 1})
    why = None
    try:
        ref = [lgo.nlpd_and_grad(kid, theta[b], X[b], y[b]) for b in check]
        if any(r[3] > 0 for r in ref):
            why = "the oracle needs jitter"
        else:
            miss = max(np.max(np.abs(r[1] - lgo.central_difference(kid, theta[b], X[b], y[b]))) / np.max(np.abs(r[1])) for b, r in zip(check, ref))
            if not miss <= SELF:
                why = f"the oracle misses its central difference: {miss:.3g} of max|grad|"
    except lo.go.NotPositiveDefinite:
        why = "the oracle's jitter ladder rejects it"
    if why:
        skipped += 1
        print(f"skipped ({why})", tag)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)
    ctx.loo_grad_reserve(B)
    rc, nlpd, grad, logml, info = ctx.loo_nll_grad_batch(X, y, theta, kid)
    for b, (onl, og, olml, _) in zip(check, ref):
        e = max(abs(nlpd[b] - onl) / abs(onl), np.max(np.abs(grad[b] - og)) / np.max(np.abs(og)))
        ok = info[b] == 0 and e <= TOL and abs(logml[b] - olml) <= 1e-9 * abs(olml)
        worst = max(worst, e / TOL) if ok else worst
        if not ok:
            print("FAIL", tag, "fit", b, "err", e, "info", info[b]); bad += 1
    ctx.close()
too_many = skipped > 0.10 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 10 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
