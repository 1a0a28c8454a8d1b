#!/usr/bin/env python3
"""Benchmark of the multi-target objective (cgp_multi_nll_grad_batch_device: value and gradient of -sum_p logml[p] from ONE
factorisation per fit) beside the only other public route to that gradient -- P calls of cgp_nll_grad per fit at the same theta,
P factorisations of the same matrix -- in one process, on the same samples (same-process A/B: one box, one clock state).  fp64,
N = 2048, d = 6, SE-ARD; the multi route device-resident with events around each call on one stream after warm-up, the column
route (host buffers, it blocks) between the same events.  Prints ONE JSON line and writes it to --out
(profiles/multi_opt_bench.json):
  shapes[]: fits, P, multi_ms, columns_ms, speedup (columns / multi), routes_max_rel_diff (nll and gradient of the two routes),
            <kernel>_ms for k_multi_solve / k_multi_alpha / k_multi_grad (device time per launch from torch.profiler; null where
            the profiler does not see the library's kernels) and their fraction of the 78.6 TFLOP/s fp64 MFMA peak by algorithmic
            flops per fit (solve P N^2, alpha P N^2, grad N^3 / 3 + P N^2)
  crossover_p: the smallest P of the lone-fit shapes from which the multi route is faster
  optimise: one cgp_optimize_multi_batch run (N = 1024, d = 1, P = 64 slip series on one time base, from all-ones): wall ms,
            evaluations, sum logml
  max_err_over_bar: the timed multi outputs of the first shape against tests/multi_opt_oracle.py on fit 0, after the timed
            regions, in units of the 1e-6 bar; the tool fails beyond 1, and when the multi route loses at 1 fit x P = 64"""
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", type=str, default="1x1,1x8,1x64,1x512,64x8")
ap.add_argument("--opt-n", type=int, default=1024)
ap.add_argument("--opt-p", type=int, default=64)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "multi_opt_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from corenav_gp_amd import synth
import multi_opt_oracle as moo   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20269)
N, d, kid = args.n, 6, engine.KERNEL_SE_ARD
shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
BMAX, PMAX = max(b for b, _ in shapes), max(p for _, p in shapes)
KERNELS = ("k_multi_solve", "k_multi_alpha", "k_multi_grad")


def timed(call, n, warm=2):
    for _ in range(warm):
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
    """device time per launch of the kernels called `names`, from one profiled call"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        res = {}
        for name in names:
            rx = re.compile(r"\b" + name + r"\s*[<(]")
            hits = [(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total, e.count)
                    for e in prof.key_averages() if rx.search(e.key)]
            res[name] = sum(v for v, _ in hits) / sum(c for _, c in hits) / 1e3 if hits else None
        return res
    except Exception:   # measurement aid only
        return {name: None for name in names}


X = rng.uniform(-2.0, 2.0, (BMAX, N, d))
W = rng.normal(size=(BMAX, d, PMAX))
Y = np.sin(X @ W).transpose(0, 2, 1) + 0.05 * rng.normal(size=(BMAX, PMAX, N))   # (B, P, N)
th = np.column_stack([rng.uniform(0.5, 1.5, BMAX)] + [rng.uniform(1.0, 3.0, BMAX) for _ in range(d)] + [np.full(BMAX, 0.01)])
thp = np.zeros((BMAX, engine.MAX_THETA))
thp[:, :d + 2] = th
dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
dY, dth = torch.from_numpy(np.ascontiguousarray(Y)).to(dev), torch.from_numpy(thp).to(dev)
multi = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=BMAX)
multi.multi_reserve(BMAX, PMAX)
multi.multi_grad_reserve(BMAX, PMAX)
single = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=1)
f64 = dict(device=dev, dtype=torch.float64)
out = {"metric": "multi-target-gradient-vs-P-column-calls", "N": N, "d": d, "kernel": "se_ard", "peak_tflops": PEAK_TFLOPS, "shapes": []}
first = None
for B, P in shapes:
    dYc = dY[:B, :P].contiguous()
    dn, dg, dl = torch.empty(B, **f64), torch.empty((B, d + 2), **f64), torch.empty((B, P), **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)

    def run_multi():
        multi.multi_nll_grad_batch_device(B, N, d, P, kid, dX.data_ptr(), dYc.data_ptr(), dth.data_ptr(), 0, dn.data_ptr(),
                                          dg.data_ptr(), d + 2, dl.data_ptr(), di.data_ptr(), stream)

    cols = {}

    def run_cols():
        for b in range(B):
            acc_n, acc_g = 0.0, 0.0
            for p in range(P):
                n1, g1 = single.nll_grad(X[b], Y[b, p], kid, th[b])
                acc_n, acc_g = acc_n + n1, acc_g + g1
            cols[b] = (acc_n, acc_g)

    rec = {"fits": B, "P": P, "multi_ms": timed(run_multi, args.reps), "columns_ms": timed(run_cols, args.reps, warm=1)}
    rec["speedup"] = rec["columns_ms"] / rec["multi_ms"]
    assert not di.cpu().numpy().any()
    hn, hg = dn.cpu().numpy(), dg.cpu().numpy()
    rec["routes_max_rel_diff"] = float(max(max(abs(hn[b] - cols[b][0]) / abs(cols[b][0]),
                                               np.max(np.abs(hg[b] - cols[b][1])) / np.max(np.abs(cols[b][1]))) for b in range(B)))
    k = kernel_ms(run_multi, KERNELS)
    flops = {"k_multi_solve": float(P) * N * N, "k_multi_alpha": float(P) * N * N, "k_multi_grad": N ** 3 / 3.0 + float(P) * N * N}
    for name in KERNELS:
        rec[name + "_ms"] = k[name]
        rec[name + "_frac_of_multi"] = k[name] / rec["multi_ms"] if k[name] else None
        rec[name + "_frac_of_peak"] = B * flops[name] / (k[name] * 1e-3) / (PEAK_TFLOPS * 1e12) if k[name] else None
    out["shapes"].append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    if first is None:
        first = (P, hn.copy(), hg.copy(), dl.cpu().numpy())
lone = sorted((r["P"], r["speedup"]) for r in out["shapes"] if r["fits"] == 1)
out["crossover_p"] = next((p for i, (p, s) in enumerate(lone) if all(s2 > 1.0 for _, s2 in lone[i:])), None)
# one full optimisation: P slip series on one time base, from all-ones
No, Po = args.opt_n, args.opt_p
t = np.arange(11, 11 + No, dtype=np.float64)
Yo = np.stack([synth._slip_series(np.random.default_rng(9000 + p), t) for p in range(Po)])
octx = engine.Context(max_n=No, max_m=No, max_d=1, max_batch=1)
octx.multi_reserve(1, Po)
octx.multi_grad_reserve(1, Po)
octx.optimize_multi_batch(t[None, :, None], Yo[None], kid, np.ones(3), max_evals=2)   # warm-up
t0 = time.perf_counter()
tho, lmlo, nevo = octx.optimize_multi_batch(t[None, :, None], Yo[None], kid, np.ones(3))
out["optimise"] = {"N": No, "d": 1, "P": Po, "wall_ms": (time.perf_counter() - t0) * 1e3, "evaluations": int(nevo[0]),
                   "sum_logml": float(lmlo[0]), "theta": tho[0].tolist()}
P, hn, hg, hl = first
onll, og, ol = moo.nll_and_grad_multi(kid, th[0], X[0], Y[0, :P])
out["max_err_over_bar"] = float(max(abs(hn[0] - onll) / abs(onll), np.max(np.abs(hg[0] - og)) / np.max(np.abs(og)),
                                    np.max(np.abs(hl[0] - ol) / np.maximum(1.0, np.abs(ol))))) / 1e-6
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
must_win = [r for r in out["shapes"] if (r["fits"], r["P"]) == (1, 64)]
sys.exit(0 if out["max_err_over_bar"] <= 1.0 and all(r["speedup"] > 1.0 for r in must_win) else 1)
