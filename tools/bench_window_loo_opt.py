#!/usr/bin/env python3
"""Benchmark of the windows' leave-one-out objective beside the only routes without it, in one process, on the same samples
(same-process A/B: one box, one clock state).  `--windows` windows x N = 512, d = 3, SE-ARD, filled and advanced by 40 ticks; fp64;
medians of `--reps`, events on the stream.  Prints ONE JSON line:
  loo_ms, nll_grad_ms            cgp_window_loo_device (lpd_sum only) and cgp_window_nll_grad_device on the same windows
  eval_ms                        (a) ONE cgp_window_loo_nll_grad_device evaluation (nine launches)
  differences_ms                 (b) the route without it on the windows: 2 ntheta rounds of cgp_window_set_theta_device +
                                 cgp_window_loo_device at theta_i (1 +- 1e-5) (the start theta is put back outside the timed region)
  mirror_ms                      (c) the host-mirror route: cgp_loo_nll_grad_batch on the same samples uploaded from the host (the
                                 blocking host call: upload, factorisation, gradient, download)
  eval_vs_differences, eval_vs_mirror     the route's time / eval_ms (> 1: the resident evaluation wins)
  optimize: ONE full optimisation from one start, at most --max-evals evaluations per window
    window_ms                    cgp_window_optimize_loo (blocking host call; the start theta is put back outside the timed region)
    mirror_ms                    cgp_optimize_loo_batch on the host mirror of the same samples
    evals_*                      mean evaluations per window of each
  max_err_over_bar               window 0 and the last window against tests/window_loo_grad_oracle.py, after the timed regions, in
                                 units of the 1e-6 bar; the tool fails beyond 1
`--only-eval K`: K evaluations of (a) and nothing else -- the run to put under a kernel trace for the per-kernel split."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--max-evals", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only-eval", type=int, default=0)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20270)
W, N, d, kid = args.windows, args.n, 3, engine.KERNEL_SE_ARD
T = N + 40
t = np.arange(11, 11 + T, dtype=np.float64)
X = np.empty((W, T, d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None, :] * rng.uniform(0.5, 1.5, (W, 1)) + rng.normal(0, 0.03, (W, T))
theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
nth = len(theta)
out = {"metric": "window-loo-opt", "windows": W, "N": N, "d": d}


def timed(call, n, before=None):
    ms = []
    for i in range(n + 2):
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if i >= 2:   # two warm-up calls
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, kid, theta)
ctx.window_loo_grad_reserve()
ctx.window_push(X, y)
f = lambda *s: torch.empty(s, device=dev, dtype=torch.float64)
dn, dg, dl, ds = f(W), f(W, nth), f(W), f(W)
evaluate = lambda: ctx.window_loo_nll_grad_device(dn.data_ptr(), dg.data_ptr(), nth, dl.data_ptr(), stream)
if args.only_eval:
    for _ in range(args.only_eval):
        evaluate()
    torch.cuda.synchronize()
    sys.exit(0)
out["loo_ms"] = timed(lambda: ctx.window_loo_device(0, 0, 0, ds.data_ptr(), stream), args.reps)
out["nll_grad_ms"] = timed(lambda: ctx.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), nth, stream), args.reps)
out["eval_ms"] = timed(evaluate, args.reps)

# (b) central differences through set_theta + window_loo
trial = []
for i in range(nth):
    for sgn in (1.0, -1.0):
        th = np.tile(theta, (W, 1))
        th[:, i] *= 1.0 + sgn * 1e-5
        trial.append(torch.from_numpy(th).to(dev))
dinfo = torch.zeros(W, device=dev, dtype=torch.int32)


def differences():
    for th in trial:
        ctx.window_set_theta_device(th.data_ptr(), nth, 0, 0, dinfo.data_ptr(), stream)
        ctx.window_loo_device(0, 0, 0, ds.data_ptr(), stream)


out["differences_ms"] = timed(differences, max(2, args.reps // 2))
ctx.window_set_theta(theta)

# (c) the host mirror
batch = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
batch.loo_grad_reserve(W)
mX, my = np.ascontiguousarray(X[:, T - N:]), np.ascontiguousarray(y[:, T - N:])
thetas = np.tile(theta, (W, 1))
out["mirror_ms"] = timed(lambda: batch.loo_nll_grad_batch(mX, my, thetas, kid), args.reps)
out["eval_vs_differences"] = out["differences_ms"] / out["eval_ms"]
out["eval_vs_mirror"] = out["mirror_ms"] / out["eval_ms"]

# correctness of what was timed
import loo_grad_oracle as lgo   # checker only, after the timed regions
worst = 0.0
nlpd, g, logml = ctx.window_loo_nll_grad()
for w in (0, W - 1):
    fo, og, ol, _ = lgo.nlpd_and_grad(kid, theta, mX[w], my[w])
    worst = max(worst, abs(nlpd[w] - fo) / max(abs(fo), 1.0) / 1e-6, np.max(np.abs(g[w] - og)) / np.max(np.abs(og)) / 1e-6,
                abs(logml[w] - ol) / max(abs(ol), 1.0) / 1e-6)

# ---- one full optimisation ---------------------------------------------------------------------------------------------------------
start = np.concatenate([[0.05], np.ones(d), [0.01]])
res = {}
opt = {"max_evals": args.max_evals}
reps = max(2, args.reps // 2)
opt["window_ms"] = timed(lambda: res.__setitem__("window", ctx.window_optimize_loo(max_evals=args.max_evals)), reps,
                         before=lambda: ctx.window_set_theta(start))
opt["mirror_ms"] = timed(lambda: res.__setitem__("mirror", batch.optimize_loo_batch(mX, my, kid, start, max_evals=args.max_evals)), reps)
opt["evals_window"] = float(np.mean(res["window"][2]))
opt["evals_mirror"] = float(np.mean(res["mirror"][3]))
opt["window_vs_mirror"] = opt["mirror_ms"] / opt["window_ms"]
opt["lpd_sum_gap"] = float(np.max(np.abs(res["window"][1] - res["mirror"][1]) / np.maximum(1.0, np.abs(res["mirror"][1]))))
out["optimize"] = opt
out["max_err_over_bar"] = worst
print(json.dumps(out))
sys.exit(0 if worst <= 1.0 else 1)
