#!/usr/bin/env python3
"""Benchmark of the hyper-parameters of the resident sliding windows replaced and re-estimated in place, at the configs[3] size:
W windows x N = 512, d = 3, fp64, filled and advanced by `--ticks` steady-state ticks, device-resident, events on the stream.
Each new call is reported beside the route it replaces, timed in this process on the same samples.  Prints ONE JSON line:
  window_set_theta_ms, _frac_of_fp64_mfma_peak     cgp_window_set_theta_device: new theta, factor rebuilt (n^3 / 3 flops per window)
  window_set_theta_refit_ms, window_set_theta_vs_refit   cgp_fit_predict_batch_device at M = 64 on a copy of the windows' samples / ratio (> 1: set_theta is faster)
  window_nll_grad_ms, _frac_of_fp64_mfma_peak      cgp_window_nll_grad_device: value and gradient from the resident factor (2 n^3 / 3 flops)
  window_optimize_ms, window_optimize_evals, window_optimize_ms_per_eval     cgp_window_optimize, `--evals` evaluations per window at most (wall clock)
  batch_optimize_ms, batch_optimize_ms_per_eval    cgp_optimize_batch on a host copy of the same samples, same start and cap (wall clock: its
                                                   rounds are the batch gradient schedule; needs a context with max_m >= N)
  window_optimize_vs_batch                         batch_optimize_ms_per_eval / window_optimize_ms_per_eval (> 1: the windows are faster)
  reinit_repush_ms, window_optimize_vs_repush      cgp_window_init + N ticks pushed again (what a caller had to do to change theta at all) / ratio
  *_max_rel_err_vs_oracle                          outputs of the calls against a from-scratch refit (oracle/) on two windows, before anything is timed"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--d", type=int, default=3)
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--evals", type=int, default=5)
ap.add_argument("--no-routes", action="store_true", help="time the new calls only (profiling runs)")
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from oracle import gp_oracle as go   # checker only, before the timed regions
dev = torch.device("cuda", 0)
W, N, d, T = args.windows, args.n, args.d, args.ticks
rng = np.random.default_rng(20265)
t = np.arange(11, 11 + N + T, dtype=np.float64)
X = np.empty((W, len(t), d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, len(t), d - 1))
y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, len(t)))
theta0 = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
theta1 = np.concatenate([[0.03], np.linspace(1.5, 0.9, d), [2e-3]])
nth = len(theta0)
dX, dy = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
stream = torch.cuda.current_stream().cuda_stream


def push(c, a, b):
    xs, ys = dX[:, a:b].contiguous(), dy[:, a:b].contiguous()
    o = torch.empty((3, W, b - a), device=dev, dtype=torch.float64)
    c.window_push_device(b - a, xs.data_ptr(), ys.data_ptr(), True, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream)


def timed(call, n):
    for _ in range(2):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, 1, theta0)
push(ctx, 0, N + T)
torch.cuda.synchronize()
assert ctx.window_state(0) == (N, 0)
L = len(t)
Xw, yw = X[:, L - N:], y[:, L - N:]       # the samples the windows hold now
dth = torch.from_numpy(np.tile(theta1, (W, 1))).to(dev)
dlm, dinfo = torch.empty(W, device=dev, dtype=torch.float64), torch.empty(W, device=dev, dtype=torch.int32)
dnll, dgrad = torch.empty(W, device=dev, dtype=torch.float64), torch.empty((W, nth), device=dev, dtype=torch.float64)
set_theta = lambda: ctx.window_set_theta_device(dth.data_ptr(), nth, 0, dlm.data_ptr(), dinfo.data_ptr(), stream)
nll_grad = lambda: ctx.window_nll_grad_device(dnll.data_ptr(), dgrad.data_ptr(), nth, stream)
# ---- checked against the oracle before anything is timed
set_theta()
nll_grad()
torch.cuda.synchronize()
assert int(dinfo.abs().max().item()) == 0
e_lm = e_nll = e_g = 0.0
for w in sorted({0, W - 1}):
    onll, og = go.nll_and_grad(1, theta1, Xw[w], yw[w])
    e_lm = max(e_lm, abs(dlm[w].item() + onll) / abs(onll))
    e_nll = max(e_nll, abs(dnll[w].item() - onll) / abs(onll))
    e_g = max(e_g, float(np.max(np.abs(dgrad[w].cpu().numpy() - og)) / np.max(np.abs(og))))
out = {"metric": "window-refactors/s", "windows": W, "N": N, "d": d,
       "window_set_theta_max_rel_err_vs_oracle": e_lm, "window_nll_max_rel_err_vs_oracle": e_nll, "window_grad_max_rel_err_vs_oracle": e_g}
assert max(e_lm, e_nll, e_g) < 1e-6, out
# ---- the two device calls
ms_set = timed(set_theta, args.reps)
ms_grad = timed(nll_grad, args.reps)
out.update({"window_set_theta_ms": ms_set, "window_set_theta_frac_of_fp64_mfma_peak": W * N ** 3 / 3.0 / (ms_set * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12),
            "window_nll_grad_ms": ms_grad, "window_nll_grad_frac_of_fp64_mfma_peak": W * 2.0 * N ** 3 / 3.0 / (ms_grad * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12)})
# ---- the optimiser: back to theta0, then `--evals` evaluations per window at most
ctx.window_set_theta(theta0)
start = -ctx.window_nll_grad()[0]
t0 = time.perf_counter()
th, lml, nev = ctx.window_optimize(max_evals=args.evals)
ms_opt = (time.perf_counter() - t0) * 1e3
assert np.all(lml >= start - 1e-9 * np.abs(start)) and np.all(th > 0)
for w in sorted({0, W - 1}):
    ol = go.fit(1, th[w], Xw[w], yw[w]).logml
    assert abs(lml[w] - ol) <= 1e-6 * abs(ol), (w, lml[w], ol)
out.update({"window_optimize_ms": ms_opt, "window_optimize_evals": int(nev.max()), "window_optimize_ms_per_eval": ms_opt / int(nev.max()),
            "window_optimize_mean_logml_gain": float(np.mean(lml - start))})
if not args.no_routes:
    # ---- the refit route for set_theta: fit + M = 64 predictions of a copy of the windows' samples
    M = 64
    rctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=W)
    dXw = torch.from_numpy(np.ascontiguousarray(Xw.transpose(0, 2, 1))).to(dev)
    dyw = torch.from_numpy(np.ascontiguousarray(yw)).to(dev)
    dXs = torch.from_numpy(np.ascontiguousarray(Xw[:, -M:].transpose(0, 2, 1))).to(dev)
    thp = np.zeros((W, engine.MAX_THETA))
    thp[:, :nth] = theta1
    dthp = torch.from_numpy(thp).to(dev)
    rm, rv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    rl, ri = torch.empty(W, device=dev, dtype=torch.float64), torch.zeros(W, device=dev, dtype=torch.int32)
    ms_refit = timed(lambda: rctx.fit_predict_batch_device(W, N, d, M, 1, dXw.data_ptr(), dyw.data_ptr(), dXs.data_ptr(), dthp.data_ptr(), 0, True,
                                                           rm.data_ptr(), rv.data_ptr(), rl.data_ptr(), ri.data_ptr(), stream), 5)
    rctx.close()
    out.update({"window_set_theta_refit_ms": ms_refit, "window_set_theta_vs_refit": ms_refit / ms_set})
    # ---- the batch optimiser on a host copy: its rounds are the batch gradient schedule
    bctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=W)
    Xh, yh = np.ascontiguousarray(Xw), np.ascontiguousarray(yw)
    bctx.optimize_batch(Xh[:W], yh[:W], 1, theta0, max_evals=1)   # warm
    t0 = time.perf_counter()
    bth, blml, bnev = bctx.optimize_batch(Xh, yh, 1, theta0, max_evals=args.evals)
    ms_b = (time.perf_counter() - t0) * 1e3
    bctx.close()
    out.update({"batch_optimize_ms": ms_b, "batch_optimize_evals": int(bnev.max()), "batch_optimize_ms_per_eval": ms_b / int(bnev.max()),
                "window_optimize_vs_batch": (ms_b / int(bnev.max())) / (ms_opt / int(nev.max())),
                "window_optimize_max_rel_diff_logml_vs_batch": float(np.max(np.abs(lml - blml) / np.abs(blml)))})
    # ---- what changing theta cost before: a new cgp_window_init and the window's N ticks pushed again
    c2 = engine.Context(max_n=8, max_m=8, max_d=d)
    c2.window_init(W, N, d, 1, theta0)
    push(c2, T, N + T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c2.window_init(W, N, d, 1, theta1)
    push(c2, T, N + T)
    torch.cuda.synchronize()
    ms_re = (time.perf_counter() - t0) * 1e3
    c2.close()
    out.update({"reinit_repush_ms": ms_re, "window_set_theta_vs_repush": ms_re / ms_set, "window_optimize_vs_repush": ms_re / ms_opt})
out["value"] = W / (ms_set * 1e-3)
print(json.dumps(out))
