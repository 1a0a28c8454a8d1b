#!/usr/bin/env python3
"""Benchmark of the sliding windows' multi-point forecast (cgp_window_predict_device: mean / variance at M test points per window
from the resident factor, z = L^-1 y and inputs) at the configs[3] size: W windows x N = 512, d = 3, fp64, filled and advanced by
`--ticks` steady-state ticks, then forecast at M = 599 (the reference's 600-tick horizon) and M = 64, device-resident, events on
the stream.  Prints ONE JSON line:
  window_forecasts_per_s, window_forecast_ms          windows per second / time of one call (M = 599; `_m64` for M = 64)
  window_forecast_frac_of_fp64_mfma_peak              n^2 M flops per window / time / 78.6 TFLOP/s
  window_forecast_hbm_frac                            the factor's bytes ONCE per window (n^2/2 x 8 B) / time / 8 TB/s; the chunks of
                                                      a window (32 test points each) re-read it from their XCD's L2
  window_forecast_vs_refit                            time of cgp_fit_predict_batch_device on the same windows' samples and test
                                                      points in this process / time of the forecast (> 1: the forecast is faster) --
                                                      the route a caller had before, with a host mirror of every window
  window_forecast_max_rel_err_vs_oracle               the timed call's outputs against a from-scratch refit (oracle/) on two windows
  window_forecast_host_ms_one_window                  one N = 512 window, M = 599, host buffers in and out (cgp_window_predict)
  window_ticks_per_s                                  the pushes in front of it (the push path, for reference)"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6
HBM_PEAK_GBPS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--d", type=int, default=3)
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from oracle import gp_oracle as go   # checker only, after the timed regions
dev = torch.device("cuda", 0)
W, N, d, T, Ms = args.windows, args.n, args.d, args.ticks, (599, 64)
rng = np.random.default_rng(20264)
t = np.arange(11, 11 + N + T, dtype=np.float64)
X = np.empty((W, len(t), d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, len(t), d - 1))
y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, len(t)))
theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, 1, theta)
dX, dy = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
stream = torch.cuda.current_stream().cuda_stream


def push(a, b):
    xs, ys = dX[:, a:b].contiguous(), dy[:, a:b].contiguous()
    out = torch.empty((3, W, b - a), device=dev, dtype=torch.float64)
    ctx.window_push_device(b - a, xs.data_ptr(), ys.data_ptr(), True, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)


def timed(call, n):
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


push(0, N)
torch.cuda.synchronize()
t0 = time.perf_counter()
push(N, N + T)
torch.cuda.synchronize()
out = {"metric": "window-forecasts/s", "window_ticks_per_s": W * T / (time.perf_counter() - t0), "windows": W, "N": N, "d": d}
assert ctx.window_state(0)[1] == 0
L = len(t)
dXw = torch.from_numpy(np.ascontiguousarray(X[:, L - N:].transpose(0, 2, 1))).to(dev)   # the samples the windows hold now, [W][d][N]
dyw = torch.from_numpy(np.ascontiguousarray(y[:, L - N:])).to(dev)
thp = np.zeros((W, engine.MAX_THETA))
thp[:, :len(theta)] = theta
dth = torch.from_numpy(thp).to(dev)
for M in Ms:
    Xs = np.empty((W, M, d))
    Xs[:, :, 0] = ((t[-1] + 1 + np.arange(M)) - t.mean()) / t.std()     # the ticks after the last sample
    Xs[:, :, 1:] = rng.normal(size=(W, M, d - 1))
    dXs = torch.from_numpy(Xs).to(dev)
    dm, dv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    ms = timed(lambda: ctx.window_predict_device(M, dXs.data_ptr(), True, dm.data_ptr(), dv.data_ptr(), stream), args.reps)
    rctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=W)       # the refit route on the same samples and test points
    dXsT = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
    rm, rv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    rl, ri = torch.empty(W, device=dev, dtype=torch.float64), torch.zeros(W, device=dev, dtype=torch.int32)
    rms = timed(lambda: rctx.fit_predict_batch_device(W, N, d, M, 1, dXw.data_ptr(), dyw.data_ptr(), dXsT.data_ptr(), dth.data_ptr(), 0, True,
                                                      rm.data_ptr(), rv.data_ptr(), rl.data_ptr(), ri.data_ptr(), stream), 5)
    mean, var = dm.cpu().numpy(), dv.cpu().numpy()
    err = 0.0
    for w in sorted({0, W - 1}):
        omu, ovar = go.predict(go.fit(1, theta, X[w, L - N:], y[w, L - N:]), Xs[w])
        err = max(err, float(np.max(np.abs(mean[w] - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(var[w] - ovar) / ovar)))
    vs = float(max(np.max(np.abs(mean - rm.cpu().numpy())) / np.max(np.abs(mean)), np.max(np.abs(var - rv.cpu().numpy()) / var)))
    rctx.close()
    sfx = "" if M == Ms[0] else f"_m{M}"
    out.update({"window_forecasts_per_s" + sfx: W / (ms * 1e-3), "window_forecast_ms" + sfx: ms,
                "window_forecast_frac_of_fp64_mfma_peak" + sfx: W * float(N) * N * M / (ms * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12),
                "window_forecast_hbm_frac" + sfx: W * (N * N / 2 * 8) / (ms * 1e-3) / (HBM_PEAK_GBPS * 1e9),
                "window_forecast_refit_ms" + sfx: rms, "window_forecast_vs_refit" + sfx: rms / ms,
                "window_forecast_max_rel_err_vs_oracle" + sfx: err, "window_forecast_max_rel_diff_vs_refit_route" + sfx: vs})
c1 = engine.Context(max_n=8, max_m=8, max_d=d)
c1.window_init(1, N, d, 1, theta)
c1.window_push(X[:1, :N], y[:1, :N])
Xh = np.ascontiguousarray(X[:1, N:N + Ms[0]]) if T >= Ms[0] else np.ascontiguousarray(np.resize(X[:1, N:], (1, Ms[0], d)))
for _ in range(3):
    c1.window_predict(Xh)
t1 = time.perf_counter()
for _ in range(20):
    c1.window_predict(Xh)
out["window_forecast_host_ms_one_window"] = (time.perf_counter() - t1) / 20 * 1e3
out["value"] = out["window_forecasts_per_s"]
print(json.dumps(out))
