#!/usr/bin/env python3
"""Randomised sweep of the windows' leave-one-out objective (cgp_window_loo_nll_grad: k_window_loo's launches, k_window_loo_prep,
k_window_loo_kinv, k_window_loo_beta, k_window_loo_grad, the finish) against tests/window_loo_grad_oracle.py (test
infrastructure: uses oracle/), with the generator of tests/fuzz/fuzz_window_adapt.py: random kernel, window length N (around the
16-row block boundaries, the 64-row super-tiles and the forms above 512), input dimension, number of windows, a stream cut into
pushes at random.  After every push the theta of all or of a random subset of the windows may be replaced (cgp_window_set_theta),
then value, gradient and logml of the watched windows are compared -- empty, filling, full, either side of a ring compaction, n
growing and the theta changing inside ONE reservation.  Also checked per evaluation: nlpd is bitwise -cgp_window_loo's sum, and
logml = NULL leaves nlpd and the gradient identical.  The windows have no jitter ladder: a drawn case is skipped only when the
oracle's fit of some watched window needed jitter or raised NotPositiveDefinite; the last line says how many were, and more than
5 % of the drawn cases skipped is a failure.
   python tests/fuzz/fuzz_window_loo_grad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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
import window_loo_grad_oracle as wo

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 129, 200]
BAR = 1e-6
t_end, cases, bad, skipped, worst = time.time() + budget, 0, 0, 0, 0.0


def base_theta(kid, d):
    return {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))


while time.time() < t_end and (max_cases == 0 or cases + skipped < max_cases):
    N = int(rng.choice(NS))
    if rng.integers(0, 40) == 0:
        N = int(rng.choice([513, 600, 1025, 1100]))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == synth.KERNEL_RBF_BROWNIAN else int(rng.integers(1, 7))
    T = int(rng.integers(2, 3 * N + 20)) if N <= 200 else int(rng.integers(N // 2, N + 40))
    nwin = int(rng.integers(1, 4))
    if N <= 64 and rng.integers(0, 4) == 0:
        nwin = int(rng.integers(100, 700))
    seed = int(rng.integers(0, 1 << 30))
    Xw, yw = [], []
    for w in range(nwin):
        r2 = np.random.default_rng(seed + w)
        t = np.arange(11 + w, 11 + w + T, dtype=np.float64)
        y = synth._slip_series(r2, t)
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / t.std()] + [r2.normal(size=T) for _ in range(d - 1)])
        Xw.append(X); yw.append(y)
    X, y = np.stack(Xw), np.stack(yw)
    theta = np.tile(base_theta(kid, d), (nwin, 1))     # the theta in force, per window
    watch = list(range(nwin)) if nwin <= 4 else sorted({0, nwin - 1, int(rng.integers(0, nwin))})
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(0, T + 1, size=int(rng.integers(1, 4)))]))
    tag0 = f"N={N} d={d} kid={kid} T={T} nwin={nwin} cuts={cuts} seed={seed}"
    # the plan: (cut, select or None, new theta or None) and the oracle's answers, before anything runs on the GPU
    plan, refs = [], []
    try:
        for b in cuts:
            op = int(rng.integers(0, 3))
            sel, new = None, None
            if op in (0, 1):
                sel = np.ones(nwin, dtype=bool) if op == 0 else rng.random(nwin) < 0.5
                new = theta * np.exp(rng.uniform(-0.3, 0.3, size=theta.shape))
                theta = theta.copy()
                theta[sel] = new[sel]
            plan.append((b, sel, new))
            ref = {w: wo.window_nlpd_and_grad(kid, theta[w], N, X[w], y[w], b) for w in watch}
            if any(r[3] != 0.0 for r in ref.values()):
                raise go.NotPositiveDefinite("jitter")
            refs.append(ref)
    except (go.NotPositiveDefinite, np.linalg.LinAlgError):
        skipped += 1
        print("skipped (the oracle's fit of a window needs jitter)", tag0)
        continue
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, np.tile(base_theta(kid, d), (nwin, 1)))
    ctx.window_loo_grad_reserve()
    a = 0
    for (b, sel, new), ref in zip(plan, refs):
        if b > a:
            ctx.window_push(X[:, a:b], y[:, a:b])
        a = b
        if new is not None:
            ctx.window_set_theta(new, select=sel)
        nlpd, g, logml = ctx.window_loo_nll_grad()
        n2, g2, _ = ctx.window_loo_nll_grad(want_logml=False)
        tot = ctx.window_loo()[3]
        if not (np.array_equal(nlpd, n2) and np.array_equal(g, g2) and np.array_equal(nlpd, -tot)):
            print("FAIL", tag0, "at", b, "logml = NULL moved nlpd / grad, or nlpd is not bitwise -cgp_window_loo's sum"); bad += 1
        for w in watch:
            f, og, ol, _ = ref[w]
            if b == 0:   # the empty-window rule holds exactly
                ok, e = bool(nlpd[w] == 0.0 and np.all(g[w] == 0.0) and logml[w] == 0.0), 0.0
            else:
                e = max(abs(nlpd[w] - f) / max(abs(f), 1.0), np.max(np.abs(g[w] - og)) / np.max(np.abs(og)), abs(logml[w] - ol) / max(abs(ol), 1.0))
                ok = e <= BAR
            worst = max(worst, e / BAR) if ok else worst
            if not ok:
                print("FAIL", tag0, "at", b, "window", w, "nlpd", nlpd[w], f, "grad", g[w], og, "logml", logml[w], ol); bad += 1
    ctx.close()
too_many = skipped > 0.05 * max(cases + skipped, 1)
print(f"cases {cases} failures {bad} skipped {skipped}{' (over the 5 % cap)' if too_many else ''} worst error / bar {worst:.3g}")
sys.exit(1 if bad or too_many else 0)
