#!/usr/bin/env python3
"""Benchmark of the multi-target windows' summed objective beside the only routes without it, in one process, on the same samples
(same-process A/B: one box, one clock state).  `--windows` windows x N = 512, d = 3, SE-ARD, filled and advanced by 40 ticks; fp64;
medians of `--reps`, events on the stream.  Prints ONE JSON line:
  nll_grad_ms                    cgp_window_nll_grad_device on a resident single-target set (one column)
  rows[]: one per P in --ps -- ONE evaluation
    multi_ms                     cgp_window_multi_nll_grad_device: diagonal inverses, Z = L^-1 Y, A = L^-T Z, the contraction, the finish
    replicate_ms                 (a) the replicate route: ONE resident single-target set evaluated P times by cgp_window_nll_grad_device
                                 (P sets of 1 024 x N = 512 windows are P x 8.6 GB of factors: 64 do not fit a card)
    mirror_ms                    (b) the host-mirror route: cgp_multi_nll_grad_batch on the same samples uploaded from the host (the
                                 blocking host call: upload, factorisation, gradient, download)
    multi_vs_replicate, multi_vs_mirror     the route's time / multi_ms (> 1: the resident evaluation wins)
  optimize: ONE full optimisation at P = --opt-p from one start, at most --max-evals evaluations per window
    multi_ms                     cgp_window_optimize_multi (blocking host call; the start theta is put back outside the timed region)
    mirror_ms                    cgp_optimize_multi_batch on the host mirror of the same samples
    single_ms                    cgp_window_optimize on the single-target set: what column 0 alone costs
    evals_*                      mean evaluations per window of each
  max_err_over_bar               window 0 and the last window of every P against tests/window_multi_opt_oracle.py, after the timed
                                 regions, in units of the 1e-6 bar; the tool fails beyond 1"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--ps", type=int, nargs="+", default=[1, 4, 16, 64])
ap.add_argument("--opt-p", type=int, default=4)
ap.add_argument("--max-evals", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import window_multi_oracle as wm   # checkers only, after the timed regions
import window_multi_opt_oracle as wmo
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20269)
W, N, d, kid = args.windows, args.n, 3, engine.KERNEL_SE_ARD
PMAX = max(args.ps + [args.opt_p])
T = N + 40
t = np.arange(11, 11 + T, dtype=np.float64)
X = np.empty((W, T, d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
Y = (0.1 * np.sin(2 * np.pi * t / 40.0)[None, :, None] * rng.uniform(0.5, 1.5, (W, 1, PMAX)) + rng.normal(0, 0.03, (W, T, PMAX)))
theta = wm.theta_of(kid, d)
nth = len(theta)
out = {"metric": "window-multi-opt", "windows": W, "N": N, "d": d, "rows": []}


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


def mirror_of(P):
    """the host mirror of the windows' samples, as cgp_multi_nll_grad_batch takes them"""
    return np.ascontiguousarray(X[:, T - N:]), np.ascontiguousarray(Y[:, T - N:, :P].transpose(0, 2, 1))


# ---- the single-target set: column 0 ------------------------------------------------------------------------------------------
single = engine.Context(max_n=8, max_m=8, max_d=d)
single.window_init(W, N, d, kid, theta)
single.window_push(X, Y[:, :, 0])
dn, dg = torch.empty(W, device=dev, dtype=torch.float64), torch.empty((W, nth), device=dev, dtype=torch.float64)
out["nll_grad_ms"] = timed(lambda: single.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), nth, stream), args.reps)
batch = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
batch.multi_reserve(W, PMAX)
batch.multi_grad_reserve(W, PMAX)
thetas = np.tile(theta, (W, 1))

worst = 0.0
for P in args.ps:
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    ctx.window_multi_reserve(P)
    ctx.window_multi_grad_reserve()
    ctx.window_push_multi(X, Y[:, :, :P])
    dl = torch.empty((W, P), device=dev, dtype=torch.float64)
    multi = timed(lambda: ctx.window_multi_nll_grad_device(P, dn.data_ptr(), dg.data_ptr(), nth, dl.data_ptr(), stream), args.reps)

    def replicate():
        for _ in range(P):
            single.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), nth, stream)
    rep = timed(replicate, max(2, args.reps // 2)) if P > 1 else out["nll_grad_ms"]
    mX, mY = mirror_of(P)
    mirror = timed(lambda: batch.multi_nll_grad_batch(mX, mY, thetas, kid), args.reps)
    out["rows"].append({"P": P, "multi_ms": multi, "replicate_ms": rep, "mirror_ms": mirror, "multi_vs_replicate": rep / multi,
                        "multi_vs_mirror": mirror / multi})
    # correctness of what was timed
    nll, g, logml = ctx.window_multi_nll_grad()
    for w in (0, W - 1):
        onll, og, ol = wmo.nll_and_grad_multi(kid, theta, N, X[w], Y[w, :, :P])
        worst = max(worst, abs(nll[w] - onll) / max(abs(onll), 1.0) / 1e-6, np.max(np.abs(g[w] - og)) / np.max(np.abs(og)) / 1e-6,
                    np.max(np.abs(logml[w] - ol) / np.maximum(1.0, np.abs(ol))) / 1e-6)
    ctx.close()
    del dl
    torch.cuda.empty_cache()

# ---- one full optimisation ---------------------------------------------------------------------------------------------------------
P = args.opt_p
start = np.concatenate([[0.05], np.ones(d), [0.01]])
ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, kid, start)
ctx.window_multi_reserve(P)
ctx.window_multi_grad_reserve()
ctx.window_push_multi(X, Y[:, :, :P])
res = {}
opt = {"P": P, "max_evals": args.max_evals}
reps = max(2, args.reps // 2)
opt["multi_ms"] = timed(lambda: res.__setitem__("multi", ctx.window_optimize_multi(max_evals=args.max_evals)), reps,
                        before=lambda: ctx.window_set_theta(start))
mX, mY = mirror_of(P)
opt["mirror_ms"] = timed(lambda: res.__setitem__("mirror", batch.optimize_multi_batch(mX, mY, kid, start, max_evals=args.max_evals)), reps)
opt["single_ms"] = timed(lambda: res.__setitem__("single", single.window_optimize(max_evals=args.max_evals)), reps,
                         before=lambda: single.window_set_theta(start))
for k in ("multi", "mirror", "single"):
    opt["evals_" + k] = float(np.mean(res[k][2]))
opt["multi_vs_mirror"] = opt["mirror_ms"] / opt["multi_ms"]
opt["logml_sum_gap"] = float(np.max(np.abs(res["multi"][1] - res["mirror"][1]) / np.maximum(1.0, np.abs(res["mirror"][1]))))
out["optimize"] = opt
out["max_err_over_bar"] = worst
print(json.dumps(out))
sys.exit(0 if worst <= 1.0 else 1)
