#!/usr/bin/env python3
"""Randomised sweep of the multi-target objective (cgp_multi_nll_grad_batch: the gradient-mode fit schedules, k_multi_pack,
k_multi_solve in both tile heights, k_multi_logml, k_multi_alpha, k_multi_grad, k_multi_grad_finish) against the per-column oracle
(tests/multi_opt_oracle.py; test infrastructure: uses oracle/): random kernel (all five), window length N <= 301 (around the
16- and 128-column boundaries), input dimension, number of targets P <= 129 with P N <= 9000 (around the 16-, 64- and 128-row boundaries; the
oracle costs one N^3 evaluation per column), batch <= 4.  The last fit of every call is checked: nll, gradient and logml at the project's 1e-6.  No case is dropped: an oracle
that raises ends the sweep with its exception.
   python tests/fuzz/fuzz_multi_opt.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
oracle-only: no GPU -- draws the same cases and runs the oracle alone."""
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
import multi_opt_oracle as moo

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [1, 2, 15, 16, 17, 63, 65, 100, 127, 128, 129, 134, 200, 255, 256, 257, 301]
PS = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128, 129]
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases < max_cases):
    N = int(rng.choice(NS))
    P = int(rng.choice([p for p in PS if p * N <= 9000]))   # the oracle is one N^3 evaluation per column
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 7))
    B = int(rng.integers(1, 5))
    form = int(rng.choice([0, 64, 128]))
    seed = int(rng.integers(0, 1 << 30))
    Xw, Yw = [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1) + b), t) for p in range(P)])
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=N) for _ in range(d - 1)])
        Xw.append(X); Yw.append(Y)
    X, Y = np.stack(Xw), np.stack(Yw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (B, 1)) * (1.0 + 0.2 * rng.random((B, 1)))
    tag = f"N={N} d={d} kid={kid} B={B} P={P} form={form} seed={seed}"
    b = B - 1
    onll, og, ol = moo.nll_and_grad_multi(kid, theta[b], X[b], Y[b])
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)
    ctx.multi_reserve(B, P)
    ctx.multi_grad_reserve(B, P)
    ctx.multi_set_form(form)
    rc, nll, grad, logml, info = ctx.multi_nll_grad_batch(X, Y, theta, kid)
    e = float(max(abs(nll[b] - onll) / abs(onll), np.max(np.abs(grad[b] - og)) / np.max(np.abs(og)),
                  np.max(np.abs(logml[b] - ol) / np.maximum(1.0, np.abs(ol)))))
    worst = max(worst, e / 1e-6)
    if not (e < 1e-6) or info.any() or rc != 0:
        print("FAIL", tag, "fit", b, "err", e, "info", info, "rc", rc); bad += 1
    ctx.close()
print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
sys.exit(1 if bad else 0)
