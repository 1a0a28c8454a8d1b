#!/usr/bin/env python3
"""Randomised sweep of the windows' hyper-parameters replaced in place (cgp_window_set_theta: k_window_refactor;
cgp_window_nll_grad: k_window_alpha + k_window_kinv_grad) against the refit oracle (test infrastructure: uses oracle/): random
kernel, window length N (around the 16-row block boundaries and the three forms of the refactor), input dimension, number of
windows; pushes, set_theta (of all or of a random subset of the windows), nll_grad and forecasts interleaved at random --
empty, filling, full, either side of a ring compaction -- each checked against a from-scratch refit of the window's samples
under the theta in force for that window.
   python tests/fuzz/fuzz_window_adapt.py [seconds=60] [seed=0]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
from corenav_gp_amd import engine, synth
from oracle import gp_oracle as go
from adapt_oracle import stream_ticks, window_logml, window_nll_grad
from forecast_oracle import sliding_window_forecast

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
NS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100, 129, 200]
BAR = 1e-6
t_end, cases, bad, worst = time.time() + budget, 0, 0, 0.0


def base_theta(kid, d):
    return {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]),
            1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]


def note(e, tag):
    global bad, worst
    worst = max(worst, e / BAR)
    if not (e < BAR):
        print("FAIL", tag, "err", e); bad += 1


while time.time() < t_end:
    N = int(rng.choice(NS))
    if rng.integers(0, 40) == 0:
        N = int(rng.choice([513, 600, 1025, 1100]))     # the eight- and sixteen-accumulator forms
    kid = int(rng.integers(0, 3))
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
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, theta)
    watch = list(range(nwin)) if nwin <= 4 else sorted({0, nwin - 1, int(rng.integers(0, nwin))})
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(0, T + 1, size=int(rng.integers(1, 5)))]))
    tag0 = f"N={N} d={d} kid={kid} T={T} nwin={nwin} cuts={cuts} seed={seed}"
    a = 0
    for b in cuts:
        if b > a:
            out = ctx.window_push(X[:, a:b], y[:, a:b])
            k = min(b - a, 3)                           # the first ticks after whatever happened at `a`
            for w in watch:
                ref = stream_ticks(kid, theta[w], N, X[w], y[w], a, a + k)
                for o, r, sc in zip(out, ref, (max(np.max(np.abs(ref[0])), np.max(np.sqrt(ref[1]))), None, None)):
                    e = np.max(np.abs(o[w, :k] - r)) / sc if sc is not None else np.max(np.abs(o[w, :k] - r) / np.maximum(np.abs(r), 1e-12))
                    note(float(e), f"push {tag0} at={a} window {w}")
            cases += 1
        a = b
        op = int(rng.integers(0, 4))
        if op in (0, 1):                                # set_theta of all windows or of a subset
            sel = np.ones(nwin, dtype=bool) if op == 0 else rng.random(nwin) < 0.5
            new = theta * np.exp(rng.uniform(-0.5, 0.5, size=theta.shape))
            logml, info = ctx.window_set_theta(new, select=None if op == 0 else sel)
            theta[sel] = new[sel]
            cases += 1
            for w in watch:
                if sel[w]:
                    ol = window_logml(kid, theta[w], N, X[w], y[w], b)
                    note(abs(logml[w] - ol) / max(abs(ol), 1.0), f"set_theta {tag0} at={b} window {w}")
                if info[w] != 0 or ctx.window_state(w) != (min(N, b), 0):
                    print("FAIL state", tag0, b, w, info[w], ctx.window_state(w)); bad += 1
        elif op == 2:
            nll, g = ctx.window_nll_grad()
            cases += 1
            for w in watch:
                onll, og = window_nll_grad(kid, theta[w], N, X[w], y[w], b)
                note(abs(nll[w] - onll) / max(abs(onll), 1.0), f"nll {tag0} at={b} window {w}")
                note(float(np.max(np.abs(g[w] - og)) / max(np.max(np.abs(og)), 1e-12)), f"grad {tag0} at={b} window {w}")
        else:
            M = int(rng.choice([1, 16, 33, 100]))
            if kid == 2:
                Xs = X[:, max(b, 1) - 1:max(b, 1), :] + 1.0 + np.arange(M, dtype=np.float64)[None, :, None] + np.zeros((nwin, 1, 1))
            else:
                Xs = X[:, rng.integers(max(0, b - N), max(b, 1), size=M)] + 0.3 * rng.normal(size=(nwin, M, d))
            mean, var = ctx.window_predict(Xs)
            cases += 1
            for w in watch:
                omu, ovar = sliding_window_forecast(kid, theta[w], N, X[w, :b], y[w, :b], Xs[w])
                note(max(float(np.max(np.abs(mean[w] - omu)) / max(np.max(np.abs(omu)), 1e-12)), float(np.max(np.abs(var[w] - ovar) / ovar))),
                     f"forecast {tag0} at={b} window {w}")
    ctx.close()
print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
sys.exit(1 if bad else 0)
