#!/usr/bin/env python3
"""Benchmark of the multi-target fits beside the route a caller had without them -- cgp_fit_predict_batch_device with batch x P
fits and X replicated -- in one process, on the same samples (same-process A/B: one box, one clock state).  fp64, N = 2048, d = 6,
M = 599, SE-ARD, device-resident, events around each call on one stream after warm-up.  Prints ONE JSON line and writes it to
--out (profiles/multi_bench.json):
  shapes[]: fits, P, multi_ms, replicate_ms, speedup (replicate / multi),
            k_multi_solve_ms, k_multi_mean_ms (device time per launch from torch.profiler; null where the profiler does not see
            the library's kernels), their fraction of the 78.6 TFLOP/s fp64 MFMA peak by algorithmic flops (P N^2 and 2 N M P per
            fit, from the real P and N)
  crossover_p: the smallest P of the lone-fit shapes from which the multi route is faster
  max_err_over_bar: the timed multi outputs of the first shape against tests/multi_oracle.py on fit 0, after the timed regions, in
            units of the 1e-6 bar; the tool fails beyond 1, and when the multi route loses at 1 fit x P = 512 or 64 fits x P = 8"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--m", type=int, default=599)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lone", type=str, default="1,2,4,8,16,32,64,512")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "multi_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from multi_oracle import fit_predict_multi, errors   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20268)
N, M, d, kid = args.n, args.m, 6, engine.KERNEL_SE_ARD
shapes = [(1, int(p)) for p in args.lone.split(",")] + [(64, 8)]
BMAX, PMAX, RMAX = max(b for b, _ in shapes), max(p for _, p in shapes), max(b * p for b, p in shapes)


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


def kernel_ms(call, names):
    """device time per launch of the kernels whose name contains one of `names`, from one profiled call"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        res = {}
        for name in names:
            hits = [(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total, e.count)
                    for e in prof.key_averages() if name in e.key]
            res[name] = sum(v for v, _ in hits) / sum(c for _, c in hits) / 1e3 if hits else None
        return res
    except Exception:   # measurement aid only
        return {name: None for name in names}


X = rng.uniform(-2.0, 2.0, (BMAX, N, d))
Xs = rng.uniform(-2.0, 2.0, (BMAX, M, d))
W = rng.normal(size=(BMAX, d, PMAX))
Y = np.sin(X @ W).transpose(0, 2, 1) + 0.05 * rng.normal(size=(BMAX, PMAX, N))   # (B, P, N)
th = np.column_stack([rng.uniform(0.5, 1.5, BMAX)] + [rng.uniform(1.0, 3.0, BMAX) for _ in range(d)] + [np.full(BMAX, 0.01)])
thp = np.zeros((BMAX, engine.MAX_THETA))
thp[:, :d + 2] = th
dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
dXs = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
dY, dth = torch.from_numpy(np.ascontiguousarray(Y)).to(dev), torch.from_numpy(thp).to(dev)
multi = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=BMAX)
multi.multi_reserve(BMAX, PMAX)
rep = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=RMAX)
f64 = dict(device=dev, dtype=torch.float64)
out = {"metric": "multi-target-vs-replicate", "N": N, "M": M, "d": d, "kernel": "se_ard", "peak_tflops": PEAK_TFLOPS, "shapes": []}
first = None
for B, P in shapes:
    dYc = dY[:B, :P].contiguous()
    mm, mv, ml = torch.empty((B, P, M), **f64), torch.empty((B, M), **f64), torch.empty((B, P), **f64)
    mi = torch.zeros(B, device=dev, dtype=torch.int32)

    def run_multi():
        multi.fit_predict_multi_batch_device(B, N, d, M, P, kid, dX.data_ptr(), dYc.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                             mm.data_ptr(), mv.data_ptr(), ml.data_ptr(), mi.data_ptr(), stream)

    # the replicate route: fit (b, p) is its own fit with X, Xs and theta of fit b
    R = B * P
    rX = dX[:B].unsqueeze(1).expand(B, P, d, N).reshape(R, d, N).contiguous()
    rXs = dXs[:B].unsqueeze(1).expand(B, P, d, M).reshape(R, d, M).contiguous()
    rth = dth[:B].unsqueeze(1).expand(B, P, engine.MAX_THETA).reshape(R, engine.MAX_THETA).contiguous()
    ry = dYc.reshape(R, N)
    rm, rv, rl = torch.empty((R, M), **f64), torch.empty((R, M), **f64), torch.empty(R, **f64)
    ri = torch.zeros(R, device=dev, dtype=torch.int32)

    def run_rep():
        rep.fit_predict_batch_device(R, N, d, M, kid, rX.data_ptr(), ry.data_ptr(), rXs.data_ptr(), rth.data_ptr(), 0, True,
                                     rm.data_ptr(), rv.data_ptr(), rl.data_ptr(), ri.data_ptr(), stream)

    rec = {"fits": B, "P": P, "multi_ms": timed(run_multi, args.reps), "replicate_ms": timed(run_rep, args.reps)}
    rec["speedup"] = rec["replicate_ms"] / rec["multi_ms"]
    assert not mi.cpu().numpy().any() and not ri.cpu().numpy().any()
    # the two routes answer the same question: agreement of their means to rounding
    rec["routes_max_rel_diff"] = float((mm.reshape(R, M) - rm).abs().max() / rm.abs().max())
    k = kernel_ms(run_multi, ("k_multi_solve", "k_multi_mean"))
    for name, flops in (("k_multi_solve", float(B) * P * N * N), ("k_multi_mean", 2.0 * B * N * M * P)):
        rec[name + "_ms"] = k[name]
        rec[name + "_frac_of_peak"] = flops / (k[name] * 1e-3) / (PEAK_TFLOPS * 1e12) if k[name] else None
    out["shapes"].append(rec)
    if first is None:
        first = (B, P, mm.cpu().numpy(), mv.cpu().numpy(), ml.cpu().numpy())
    del rX, rXs, rth, rm, rv, rl
lone = sorted((r["P"], r["speedup"]) for r in out["shapes"] if r["fits"] == 1)
out["crossover_p"] = next((p for i, (p, s) in enumerate(lone) if all(s2 > 1.0 for _, s2 in lone[i:])), None)
B, P, mean, var, logml = first
out["max_err_over_bar"] = float(max(errors(mean[0], var[0], logml[0], *fit_predict_multi(kid, th[0], X[0], Y[0, :P], Xs[0], True)))) / 1e-6
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
must_win = [r for r in out["shapes"] if (r["fits"], r["P"]) in ((1, 512), (64, 8))]
sys.exit(0 if out["max_err_over_bar"] <= 1.0 and all(r["speedup"] > 1.0 for r in must_win) else 1)
