#!/usr/bin/env python3
"""Benchmark of leave-one-out cross-validation beside the gradient call that shares its schedule, in one process, on the same
samples (same-process A/B: one box, one clock state).  fp64.  Prints ONE JSON line:
  loo_batch_device_ms            cgp_loo_batch_device, `--full` fits x N = 2048, d = 6, device-resident, events on the stream:
                                 gradient-mode factorisation + k_loo + k_loo_sum
  loo_batch_host_ms, grad_batch_host_ms, loo_vs_grad_host
                                 cgp_loo_batch against ONE gradient-mode evaluation of the same batch (cgp_optimize_batch with
                                 max_evals = 1: the same upload, the same factorisation, then k_grad), wall clock, both from host
                                 buffers; the ratio grad / loo (> 1: LOO is faster)
  k_loo_us, k_grad_us, fit_kernels_us, k_loo_gbytes, k_loo_tbytes_per_s, k_loo_frac_of_hbm_peak
                                 device time of the kernels of those two calls from torch.profiler (per call; null where the
                                 profiler does not see the library's kernels): k_loo's bytes are the columns it reads,
                                 sum over 64-row blocks of 64 x (N - start of the block's 128-column tile) doubles per fit
  window_loo_ms, window_nll_grad_ms, window_loo_vs_grad
                                 cgp_window_loo_device and cgp_window_nll_grad_device on `--windows` windows x N = 512, d = 3, filled
                                 and advanced by 40 ticks, events on the stream; the ratio grad / loo
  *_max_err_over_bar             the timed outputs against tests/loo_oracle.py on two fits / two windows, after the timed
                                 regions, in units of the 1e-6 bar; the tool fails beyond 1"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

HBM_PEAK_TBYTES_PER_S = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--full", type=int, default=512)
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import loo_oracle as lo   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20267)
out = {"metric": "loo-vs-gradient", "full_fits": args.full, "N": args.n, "windows": args.windows}


def timed(call, n):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def wall(call, n):
    call()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def over_bar(got, want, y):
    gm, gv, gl, gs = got
    return max(np.max(np.abs(gm - want.mean)) / max(1.0, float(np.max(np.abs(y)))), np.max(np.abs(gv - want.var) / want.var),
               np.max(np.abs(gl - want.lpd) / np.maximum(1.0, np.abs(want.lpd))),
               abs(gs - want.lpd_sum) / max(1.0, float(np.sum(np.abs(want.lpd))))) / 1e-6


# ---- batch: LOO beside one gradient-mode evaluation ---------------------------------------------------------------------------------
B, N, d, kid = args.full, args.n, 6, engine.KERNEL_SE_ARD
X = rng.uniform(-2.0, 2.0, (B, N, d))
y = np.sin(X @ rng.normal(size=(B, d, 1)))[:, :, 0] + 0.05 * rng.normal(size=(B, N))
th = np.column_stack([rng.uniform(0.5, 1.5, B)] + [rng.uniform(1.0, 3.0, B) for _ in range(d)] + [np.full(B, 0.01)])
thp = np.zeros((B, engine.MAX_THETA))
thp[:, :d + 2] = th
dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
dy, dth = torch.from_numpy(y).to(dev), torch.from_numpy(thp).to(dev)
ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)
o = [torch.empty((B, N), device=dev, dtype=torch.float64) for _ in range(3)] + [torch.empty(B, device=dev, dtype=torch.float64) for _ in range(2)]
oi = torch.zeros(B, device=dev, dtype=torch.int32)


def loo_device():
    ctx.loo_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, *[t.data_ptr() for t in o], oi.data_ptr(), stream)


out["loo_batch_device_ms"] = timed(loo_device, args.reps)
res = [t.cpu().numpy() for t in o]
assert not oi.cpu().numpy().any()
host = {}


def loo_host():
    host["loo"] = ctx.loo_batch(X, y, th, kid)


def grad_host():
    host["grad"] = ctx.optimize_batch(X, y, kid, th, max_evals=1)


out["loo_batch_host_ms"] = wall(loo_host, max(2, args.reps // 2))
out["grad_batch_host_ms"] = wall(grad_host, max(2, args.reps // 2))
out["grad_batch_host_evals"] = int(host["grad"][2].max())
out["loo_vs_grad_host"] = out["grad_batch_host_ms"] / out["loo_batch_host_ms"]
assert host["loo"][0] == 0 and all(np.array_equal(a, b) for a, b in zip(host["loo"][1:5], res[:4]))   # host form = device form

# device time per kernel of one call each (torch.profiler sees the library's launches when both share one HIP runtime)
kernels = {}
try:
    from torch.profiler import profile, ProfilerActivity
    for tag, call in (("loo", loo_device), ("grad", grad_host)):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            ctx.synchronize()
            torch.cuda.synchronize()
        kernels[tag] = {e.key: (e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total, e.count)
                        for e in prof.key_averages()}
except Exception as exc:   # measurement aid only
    out["profiler_error"] = repr(exc)[:200]


def kernel_us(tag, name, exclude=()):
    hits = [(v, n) for k, (v, n) in kernels.get(tag, {}).items() if name in k and not any(x in k for x in exclude)]
    return (sum(v for v, _ in hits), sum(n for _, n in hits)) if hits else (None, 0)


k_loo_us, _ = kernel_us("loo", "k_loo", exclude=("k_loo_sum",))
k_grad_us, n_grad = kernel_us("grad", "k_grad")
fit_us = sum(v for k, (v, n) in kernels.get("loo", {}).items() if "cgp::k_" in k and "k_loo" not in k) or None
nbytes = B * 8.0 * sum(64 * (N - (e0 // 128) * 128) for e0 in range(0, N, 64))
out.update(k_loo_us=k_loo_us, k_grad_us=(k_grad_us / n_grad if k_grad_us else None), fit_kernels_us=fit_us, k_loo_gbytes=nbytes / 1e9)
if k_loo_us:
    out["k_loo_tbytes_per_s"] = nbytes / (k_loo_us * 1e-6) / 1e12
    out["k_loo_frac_of_hbm_peak"] = out["k_loo_tbytes_per_s"] / HBM_PEAK_TBYTES_PER_S
out["batch_max_err_over_bar"] = max(over_bar([r[b] for r in res[:4]], lo.loo(kid, th[b], X[b], y[b]), y[b]) for b in (0, B - 1))
ctx.close()
del dX, o

# ---- resident windows: LOO beside the gradient ---------------------------------------------------------------------------------------
W, N, d, T = args.windows, 512, 3, 40
t = np.arange(11, 11 + N + T, dtype=np.float64)
Xw = np.empty((W, len(t), d))
Xw[:, :, 0] = (t - t.mean()) / t.std()
Xw[:, :, 1:] = rng.normal(size=(W, len(t), d - 1))
yw = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, len(t)))
theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
ctx = engine.Context(max_n=8, max_m=8, max_d=d)
ctx.window_init(W, N, d, engine.KERNEL_SE_ARD, theta)
dXw, dyw = torch.from_numpy(Xw).to(dev), torch.from_numpy(yw).to(dev)
po = torch.empty((3, W, len(t)), device=dev, dtype=torch.float64)
ctx.window_push_device(len(t), dXw.data_ptr(), dyw.data_ptr(), True, po[0].data_ptr(), po[1].data_ptr(), po[2].data_ptr(), stream)
torch.cuda.synchronize()
wo = [torch.empty((W, N), device=dev, dtype=torch.float64) for _ in range(3)] + [torch.empty(W, device=dev, dtype=torch.float64)]
dn, dg = torch.empty(W, device=dev, dtype=torch.float64), torch.empty((W, d + 2), device=dev, dtype=torch.float64)
out["window_loo_ms"] = timed(lambda: ctx.window_loo_device(*[t_.data_ptr() for t_ in wo], stream), args.reps)
out["window_nll_grad_ms"] = timed(lambda: ctx.window_nll_grad_device(dn.data_ptr(), dg.data_ptr(), d + 2, stream), args.reps)
out["window_loo_vs_grad"] = out["window_nll_grad_ms"] / out["window_loo_ms"]
ctx.window_loo_device(*[t_.data_ptr() for t_ in wo], stream)
torch.cuda.synchronize()
wres = [t_.cpu().numpy() for t_ in wo]
out["window_max_err_over_bar"] = max(over_bar([r[w] for r in wres], lo.loo(engine.KERNEL_SE_ARD, theta, Xw[w, -N:], yw[w, -N:]), yw[w, -N:])
                                     for w in (0, W - 1))
print(json.dumps(out))
sys.exit(0 if max(out["batch_max_err_over_bar"], out["window_max_err_over_bar"]) <= 1.0 else 1)
