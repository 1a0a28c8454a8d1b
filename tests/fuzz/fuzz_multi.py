#!/usr/bin/env python3
"""Randomised sweep of the multi-target fits (cgp_fit_predict_multi_batch: the tiled fit schedules, k_multi_pack, k_multi_solve in
both tile heights, k_multi_mean, k_multi_logml) against one oracle refit per column (tests/multi_oracle.py; test infrastructure:
uses oracle/): random kernel (all five), window length N <= 400 (around the 16- and 128-column boundaries), input dimension,
number of test points M <= 200 and of targets P <= 200 (around the 16-, 64- and 128-row boundaries), batch <= 4, noise on / off.
No case is dropped: an oracle that raises ends the sweep with its exception.
   python tests/fuzz/fuzz_multi.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
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
from multi_oracle import fit_predict_multi, errors

budget = float(argv[0]) if len(argv) > 0 else 60.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
max_cases = int(argv[2]) if len(argv) > 2 else 0
NS = [1, 2, 15, 16, 17, 63, 65, 100, 127, 128, 129, 134, 200, 255, 256, 257, 301, 385, 400]
MS = [1, 2, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 200]
PS = [1, 2, 3, 4, 15, 16, 17, 48, 63, 64, 65, 100, 127, 128, 129, 200]
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0
while time.time() < t_end and (max_cases == 0 or cases < max_cases):
    N, M, P = int(rng.choice(NS)), int(rng.choice(MS)), int(rng.choice(PS))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 7))
    B = int(rng.integers(1, 5))
    noise = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1 << 30))
    Xw, Yw, Xsw = [], [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1) + b), t) for p in range(P)])
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=N) for _ in range(d - 1)])
        Xs = X[-1:, :] + 1.0 + np.arange(M, dtype=np.float64)[:, None] if kid == 2 else \
            X[r2.integers(max(0, N - 50), N, size=M)] + 0.3 * r2.normal(size=(M, d))
        Xw.append(X); Yw.append(Y); Xsw.append(Xs)
    X, Y, Xs = np.stack(Xw), np.stack(Yw), np.stack(Xsw)
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    theta = np.tile(th1, (B, 1))
    tag = f"N={N} d={d} kid={kid} B={B} M={M} P={P} noise={noise} seed={seed}"
    check = sorted({0, B - 1})
    ref = [fit_predict_multi(kid, theta[b], X[b], Y[b], Xs[b], noise) for b in check]
    cases += 1
    if oracle_only:
        continue
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    ctx.multi_reserve(B, P)
    rc, mean, var, logml, info = ctx.fit_predict_multi_batch(X, Y, Xs, theta, kid, include_noise=noise)
    for b, o in zip(check, ref):
        e = float(max(errors(mean[b], var[b], logml[b], *o)))
        worst = max(worst, e / 1e-6)
        if not (e < 1e-6) or info[b] != 0 or rc != 0:
            print("FAIL", tag, "fit", b, "err", e, "info", info[b], "rc", rc); bad += 1
    ctx.close()
print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
sys.exit(1 if bad else 0)
