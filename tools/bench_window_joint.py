#!/usr/bin/env python3
"""Benchmark of the sliding windows' joint forecast (cgp_window_predict_cov_device: mean and the full posterior covariance at M
test points per window; cgp_window_sample_device: S sample paths) at the configs[3] size: W windows x N = 512, d = 3, fp64,
filled and advanced by `--ticks` steady-state ticks, then M = 599 (the reference's 600-tick horizon), 256 and 64, S = 16,
device-resident, events on the stream.  Prints ONE JSON line; per M (suffix `_m256`, `_m64`; none for M = 599):
  window_joint_cov_ms, window_joint_sample_ms         time of one call
  window_joint_cov_frac_of_fp64_mfma_peak             (n^2 M + n M^2) flops per window / time / 78.6 TFLOP/s
  window_joint_sample_frac_of_fp64_mfma_peak          (n^2 M + n M^2 + M^3 / 3 + M^2 S) flops per window / time / 78.6 TFLOP/s
  window_joint_marginal_ms                            cgp_window_predict_device at the same points (the solve alone)
  window_joint_refit_ms                               cgp_fit_predict_batch_device on the same samples and points (marginals only:
                                                      the route through a host mirror, for scale)
  window_joint_max_rel_err_vs_oracle                  the timed calls' outputs (mean, covariance, paths) against a from-scratch
                                                      refit (tests/joint_oracle.py) on two windows, after the timed region"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

FP64_MFMA_PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--d", type=int, default=3)
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--paths", type=int, default=16)
ap.add_argument("--m", type=int, nargs="+", default=[599, 256, 64])
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from joint_oracle import sliding_window_joint, sample_paths   # checker only, after the timed regions
dev = torch.device("cuda", 0)
W, N, d, T, Ms, S = args.windows, args.n, args.d, args.ticks, tuple(args.m), args.paths
rng = np.random.default_rng(20265)
t = np.arange(11, 11 + N + T, dtype=np.float64)
X = np.empty((W, len(t), d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, len(t), d - 1))
y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, len(t)))
theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, 1, theta)
ctx.window_joint_reserve(max(Ms))
dX, dy = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
stream = torch.cuda.current_stream().cuda_stream


def push(a, b):
    xs, ys = dX[:, a:b].contiguous(), dy[:, a:b].contiguous()
    out = torch.empty((3, W, b - a), device=dev, dtype=torch.float64)
    ctx.window_push_device(b - a, xs.data_ptr(), ys.data_ptr(), True, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)


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


push(0, N)
push(N, N + T)
torch.cuda.synchronize()
assert ctx.window_state(0)[1] == 0
out = {"metric": "window-joint-forecasts/s", "windows": W, "N": N, "d": d, "paths": S}
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
    dxi = torch.randn((W, S, M), device=dev, dtype=torch.float64)
    dm, dv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    dc = torch.empty((W, M, M), device=dev, dtype=torch.float64)
    dp = torch.empty((W, S, M), device=dev, dtype=torch.float64)
    di = torch.zeros(W, device=dev, dtype=torch.int32)
    ms_cov = timed(lambda: ctx.window_predict_cov_device(M, dXs.data_ptr(), False, dm.data_ptr(), dc.data_ptr(), stream), args.reps)
    ms_smp = timed(lambda: ctx.window_sample_device(M, dXs.data_ptr(), S, dxi.data_ptr(), True, 1e-6, dp.data_ptr(), di.data_ptr(), stream), args.reps)
    ms_mrg = timed(lambda: ctx.window_predict_device(M, dXs.data_ptr(), False, dm.data_ptr(), dv.data_ptr(), stream), args.reps)
    rctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=W)       # the refit route on the same samples and test points
    dXsT = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
    rm, rv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    rl, ri = torch.empty(W, device=dev, dtype=torch.float64), torch.zeros(W, device=dev, dtype=torch.int32)
    ms_ref = timed(lambda: rctx.fit_predict_batch_device(W, N, d, M, 1, dXw.data_ptr(), dyw.data_ptr(), dXsT.data_ptr(), dth.data_ptr(), 0, True,
                                                         rm.data_ptr(), rv.data_ptr(), rl.data_ptr(), ri.data_ptr(), stream), 3)
    rctx.close()
    assert not di.cpu().numpy().any()
    xi = dxi.cpu().numpy()
    err = 0.0
    for w in sorted({0, W - 1}):
        mean, cov, paths = dm[w].cpu().numpy(), dc[w].cpu().numpy(), dp[w].cpu().numpy()
        omu, ocov = sliding_window_joint(1, theta, N, X[w], y[w], Xs[w], include_noise=False)
        sd = np.sqrt(np.diag(ocov))
        op = sample_paths(omu, ocov, theta[-1], 1e-6, xi[w])
        err = max(err, float(np.max(np.abs(mean - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(cov - ocov) / np.outer(sd, sd))),
                  float(np.max(np.abs(paths - op)) / np.max(np.abs(op))))
    f_cov = float(N) * N * M + float(N) * M * M
    f_smp = f_cov + M ** 3 / 3.0 + float(M) * M * S
    sfx = "" if M == Ms[0] else f"_m{M}"
    out.update({"window_joint_cov_ms" + sfx: ms_cov, "window_joint_sample_ms" + sfx: ms_smp,
                "window_joint_cov_frac_of_fp64_mfma_peak" + sfx: W * f_cov / (ms_cov * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12),
                "window_joint_sample_frac_of_fp64_mfma_peak" + sfx: W * f_smp / (ms_smp * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12),
                "window_joint_marginal_ms" + sfx: ms_mrg, "window_joint_refit_ms" + sfx: ms_ref,
                "window_joint_max_rel_err_vs_oracle" + sfx: err})
    del dc, dp, dxi
out["value"] = W / (out["window_joint_cov_ms"] * 1e-3)
print(json.dumps(out))
