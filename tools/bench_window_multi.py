#!/usr/bin/env python3
"""Benchmark of the multi-target sliding windows beside the single-target calls they extend, in one process, on the same samples
(same-process A/B: one box, one clock state).  `--windows` windows x N = 512, d = 3, SE-ARD, filled and advanced by 40 ticks; fp64;
events on the stream.  Prints ONE JSON line:
  push_ms_per_tick               cgp_window_push_device, a push of `--ticks` steady-state ticks, per tick
  rows[]: one per P in --ps
    push_multi_ms_per_tick       cgp_window_push_multi_device on the same ticks (the target store's launch in front of the push's)
    per M in --ms:
      predict_ms                 (a) cgp_window_predict_device alone
      predict_multi_ms           cgp_window_predict_multi_device: diagonal inverses, Z = L^-1 Y, the forecast with P mean rows
      replicate_ms               (b) the replicate route: P single-target forecasts one after the other.  ONE single-target set is
                                 resident and forecast P times (P sets of 1 024 x N = 512 windows are P x 8.6 GB of factors: 64 do
                                 not fit a card); its push cost is P x push_ms_per_tick
      multi_vs_replicate         replicate_ms / predict_multi_ms (> 1: the shared factor wins)
      multi_vs_single            predict_multi_ms / predict_ms (what P columns cost over one)
  max_err_over_bar               window 0 and the last window of the last P against tests/window_multi_oracle.py, after the timed
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
ap.add_argument("--ms", type=int, nargs="+", default=[64, 599])
ap.add_argument("--ticks", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import window_multi_oracle as wm   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20268)
W, N, d, kid, Tb = args.windows, args.n, 3, engine.KERNEL_SE_ARD, args.ticks
PMAX, MMAX = max(args.ps), max(args.ms)
T0 = N + 40                        # ticks before the timed regions
T = T0 + Tb * (args.reps + 2)      # + the ticks the timed pushes consume (two warm-up calls)
t = np.arange(11, 11 + T, dtype=np.float64)
X = np.empty((W, T, d))
X[:, :, 0] = (t - t.mean()) / t.std()
X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
Y = (0.1 * np.sin(2 * np.pi * t / 40.0)[None, :, None] * rng.uniform(0.5, 1.5, (W, 1, PMAX)) + rng.normal(0, 0.03, (W, T, PMAX)))
theta = wm.theta_of(kid, d)
Xs = X[:, T0 - 1:T0, :] + 0.02 * np.arange(1, MMAX + 1)[None, :, None] * np.array([1.0, 0.3, -0.2])[None, None, :]
dX, dXs = torch.from_numpy(X).to(dev), torch.from_numpy(Xs).to(dev)
fill_out = torch.empty((3, W, T0), device=dev, dtype=torch.float64)   # the tick outputs of the filling push / of a timed push
tick_out = torch.empty((3, W, Tb), device=dev, dtype=torch.float64)
out = {"metric": "window-multi", "windows": W, "N": N, "d": d, "ticks_per_push": Tb, "rows": []}


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


def slices(Ycols, lo, hi):
    """contiguous device copies of a block of ticks (made outside the timed calls)"""
    return dX[:, lo:hi].contiguous(), Ycols[:, lo:hi].contiguous()


def outs(buf):
    return [buf[k].data_ptr() for k in range(3)]


# ---- the single-target set: column 0 ------------------------------------------------------------------------------------------
single = engine.Context(max_n=8, max_m=8, max_d=d)
single.window_init(W, N, d, kid, theta)
dy0 = torch.from_numpy(np.ascontiguousarray(Y[:, :, 0])).to(dev)
bx, by = slices(dy0, 0, T0)
single.window_push_device(T0, bx.data_ptr(), by.data_ptr(), True, *outs(fill_out), stream)
blocks = [slices(dy0, lo, lo + Tb) for lo in range(T0, T, Tb)]
torch.cuda.synchronize()
po = outs(tick_out)
it = iter(blocks)
out["push_ms_per_tick"] = timed(lambda: (lambda b: single.window_push_device(Tb, b[0].data_ptr(), b[1].data_ptr(), True, *po, stream))(next(it)),
                                args.reps) / Tb
sm, sv = (torch.empty((W, MMAX), device=dev, dtype=torch.float64) for _ in range(2))
xs_of = {M: dXs[:, :M].contiguous() for M in args.ms}
single_ms = {M: timed(lambda: single.window_predict_device(M, xs_of[M].data_ptr(), True, sm.data_ptr(), sv.data_ptr(), stream), args.reps)
             for M in args.ms}

# ---- P target columns on one set ---------------------------------------------------------------------------------------------
worst = 0.0
for P in args.ps:
    dY = torch.from_numpy(np.ascontiguousarray(Y[:, :, :P])).to(dev)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, kid, theta)
    ctx.window_multi_reserve(P)
    bx, bY = slices(dY, 0, T0)
    ctx.window_push_multi_device(T0, P, bx.data_ptr(), bY.data_ptr(), True, *outs(fill_out), stream)
    torch.cuda.synchronize()
    row = {"P": P, "forecast": []}
    mean, var, logml = (torch.empty(s, device=dev, dtype=torch.float64) for s in ((W, P, MMAX), (W, MMAX), (W, P)))
    for M in args.ms:
        xs = xs_of[M]
        multi = timed(lambda: ctx.window_predict_multi_device(M, P, xs.data_ptr(), True, mean.data_ptr(), var.data_ptr(), logml.data_ptr(), stream),
                      args.reps)

        def replicate():
            for _ in range(P):
                single.window_predict_device(M, xs.data_ptr(), True, sm.data_ptr(), sv.data_ptr(), stream)
        rep = timed(replicate, max(2, args.reps // 2)) if P > 1 else single_ms[M]
        row["forecast"].append({"M": M, "predict_ms": single_ms[M], "predict_multi_ms": multi, "replicate_ms": rep,
                                "multi_vs_replicate": rep / multi, "multi_vs_single": multi / single_ms[M]})
    # correctness of what was timed, on the state the forecasts saw
    M = args.ms[0]
    xs = xs_of[M]
    ctx.window_predict_multi_device(M, P, xs.data_ptr(), True, mean.data_ptr(), var.data_ptr(), logml.data_ptr(), stream)
    torch.cuda.synchronize()
    hm, hv, hl = mean.cpu().numpy().reshape(-1)[:W * P * M].reshape(W, P, M), var.cpu().numpy().reshape(-1)[:W * M].reshape(W, M), logml.cpu().numpy()
    for w in (0, W - 1):
        ref = wm.sliding_window_forecast_multi(kid, theta, N, X[w, :T0], Y[w, :T0, :P], Xs[w, :M])
        worst = max(worst, max(wm.errors(hm[w], hv[w], hl[w], *ref)) / 1e-6)
    mblocks = [slices(dY, lo, lo + Tb) for lo in range(T0, T, Tb)]
    torch.cuda.synchronize()
    it = iter(mblocks)
    row["push_multi_ms_per_tick"] = timed(lambda: (lambda b: ctx.window_push_multi_device(Tb, P, b[0].data_ptr(), b[1].data_ptr(), True, *po, stream))(next(it)),
                                          args.reps) / Tb
    row["push_multi_vs_push"] = row["push_multi_ms_per_tick"] / out["push_ms_per_tick"]
    row["push_multi_vs_replicate"] = P * out["push_ms_per_tick"] / row["push_multi_ms_per_tick"]
    out["rows"].append(row)
    ctx.close()
    del dY, mean, var, logml
    torch.cuda.empty_cache()
out["max_err_over_bar"] = worst
print(json.dumps(out))
sys.exit(0 if worst <= 1.0 else 1)
