#!/usr/bin/env python3
"""Benchmark of the sliding windows' predictive gradients (cgp_window_predict_gradients_device: d mean / d x*, d var / d x* at M
test points per window from the resident factor, z and inputs), device-resident, device events on the stream, one process.
Shapes: 1 024 windows x N = 512 x d = 3 at M = 599 and M = 64 (the shapes of tools/bench_window_forecast.py) and 128 windows x
N = 1 024 x d = 3 at M = 64 (the sixteen-point form).  Per shape three calls are timed ALTERNATELY, `--reps` rounds of one call
each, and the median of each is reported:
  gradients   cgp_window_predict_gradients_device (three launches: diagonal inverses, alpha, the gradient form of the forecast)
  forecast    cgp_window_predict_device at the same shape (two launches)
  refit       cgp_fit_predict_grad_batch_device on the samples the windows hold: the route a caller had before, which needs a
              host mirror of every window
and the two ratios gradients / forecast and gradients / refit (< 1: the gradients from the windows are faster than the refit).
The timed gradient call's outputs are compared with the refit route's (two device paths) and, on two windows, with the oracle.
Writes the JSON to --out (default profiles/window_pgrad_bench.json) and prints it as ONE line.
--gradients-only: times the gradient call alone (for a measurement build of the library selected with env CGP_LIB, such as one
compiled with -DCGP_WPG_NO_CONTRACT, whose gradients are WRONG by design: nothing is compared)."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

FP64_MFMA_PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_pgrad_bench.json"))
ap.add_argument("--gradients-only", action="store_true")
ap.add_argument("--shapes", default="1024x512x3x599,1024x512x3x64,128x1024x3x64")
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def event_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(calls, reps):
    """calls: name -> callable.  Three warm-up rounds, then `reps` rounds of one call each in turn; the median per name."""
    for _ in range(3):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            ms[k].append(event_ms(c))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: [float(min(v)), float(max(v))] for k, v in ms.items()}


def shape_run(W, N, d, M):
    rng = np.random.default_rng(20264 + N + M)
    T = args.ticks
    t = np.arange(11, 11 + N + T, dtype=np.float64)
    L = len(t)
    X = np.empty((W, L, d))
    X[:, :, 0] = (t - t.mean()) / t.std()
    X[:, :, 1:] = rng.normal(size=(W, L, d - 1))
    y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, L))
    theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, 1, theta)
    dX, dy = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    for a, b in ((0, N), (N, L)):
        xs, ys = dX[:, a:b].contiguous(), dy[:, a:b].contiguous()
        o = torch.empty((3, W, b - a), device=dev, dtype=torch.float64)
        ctx.window_push_device(b - a, xs.data_ptr(), ys.data_ptr(), True, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream)
        torch.cuda.synchronize()
    assert ctx.window_state(0) == (N, 0)
    Xs = np.empty((W, M, d))
    Xs[:, :, 0] = ((t[-1] + 1 + np.arange(M)) - t.mean()) / t.std()     # the ticks after the last sample
    Xs[:, :, 1:] = rng.normal(size=(W, M, d - 1))
    dXs = torch.from_numpy(Xs).to(dev)
    gm, gv, fm, fv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(4))
    gdm, gdv = (torch.empty((W, M, d), device=dev, dtype=torch.float64) for _ in range(2))
    calls = {"gradients": lambda: ctx.window_predict_gradients_device(M, dXs.data_ptr(), True, gm.data_ptr(), gv.data_ptr(), gdm.data_ptr(),
                                                                      gdv.data_ptr(), stream)}
    res = {"windows": W, "N": N, "d": d, "M": M}
    if args.gradients_only:
        med, rng_ = alternate(calls, args.reps)
        res.update({"gradients_ms": med["gradients"], "gradients_ms_min_max": rng_["gradients"]})
        ctx.close()
        return res
    calls["forecast"] = lambda: ctx.window_predict_device(M, dXs.data_ptr(), True, fm.data_ptr(), fv.data_ptr(), stream)
    rctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=W)
    assert rctx.pgrad_reserve(W, M) == 0
    dXw = torch.from_numpy(np.ascontiguousarray(X[:, L - N:].transpose(0, 2, 1))).to(dev)   # the samples the windows hold, [W][d][N]
    dyw = torch.from_numpy(np.ascontiguousarray(y[:, L - N:])).to(dev)
    thp = np.zeros((W, engine.MAX_THETA))
    thp[:, :len(theta)] = theta
    dth = torch.from_numpy(thp).to(dev)
    dXsT = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
    rm, rv = (torch.empty((W, M), device=dev, dtype=torch.float64) for _ in range(2))
    rl, ri = torch.empty(W, device=dev, dtype=torch.float64), torch.zeros(W, device=dev, dtype=torch.int32)
    rdm, rdv = (torch.empty((W, M, d), device=dev, dtype=torch.float64) for _ in range(2))
    calls["refit"] = lambda: rctx.fit_predict_grad_batch_device(W, N, d, M, 1, dXw.data_ptr(), dyw.data_ptr(), dXsT.data_ptr(), dth.data_ptr(), 0,
                                                                True, rm.data_ptr(), rv.data_ptr(), rl.data_ptr(), ri.data_ptr(), rdm.data_ptr(),
                                                                rdv.data_ptr(), stream)
    med, rng_ = alternate(calls, args.reps)
    torch.cuda.synchronize()
    assert not ri.any().item()
    a, b, r, rr = gdm.cpu().numpy(), gdv.cpu().numpy(), rdm.cpu().numpy(), rdv.cpu().numpy()
    per = lambda u, v: float(np.max(np.max(np.abs(u - v), axis=(1, 2)) / np.max(np.abs(v), axis=(1, 2))))
    import window_pgrad_oracle as wo   # checker only, after the timed regions
    eo = 0.0
    for w in sorted({0, W - 1}):
        odm, odv = wo.sliding_window_gradients(1, theta, N, X[w], y[w], Xs[w])
        eo = max(eo, float(np.max(np.abs(a[w] - odm)) / np.max(np.abs(odm))), float(np.max(np.abs(b[w] - odv)) / np.max(np.abs(odv))))
    assert torch.equal(gm, fm) and torch.equal(gv, fv)     # mean / var of the gradient call are the forecast's, bitwise
    flops = W * 2.0 * N * N * M
    res.update({"gradients_ms": med["gradients"], "forecast_ms": med["forecast"], "refit_ms": med["refit"],
                "ms_min_max": rng_, "gradients_over_forecast": med["gradients"] / med["forecast"],
                "gradients_over_refit": med["gradients"] / med["refit"],
                "gradients_frac_of_fp64_mfma_peak": flops / (med["gradients"] * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12),
                "max_rel_diff_vs_refit_route_dmean": per(a, r), "max_rel_diff_vs_refit_route_dvar": per(b, rr),
                "max_rel_err_vs_oracle_two_windows": eo})
    rctx.close()
    ctx.close()
    return res


out = {"metric": "window predictive gradients, ms per call (median of %d, device events, calls alternated)" % args.reps,
       "library": os.environ.get("CGP_LIB", "shipped"), "gradients_only": bool(args.gradients_only), "shapes": []}
for s in args.shapes.split(","):
    W, N, d, M = (int(v) for v in s.split("x"))
    out["shapes"].append(shape_run(W, N, d, M))
    print("done", s, file=sys.stderr, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
