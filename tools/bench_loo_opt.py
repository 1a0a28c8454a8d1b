#!/usr/bin/env python3
"""Benchmark of the leave-one-out objective (cgp_loo_nll_grad_batch_device: nlpd = -lpd_sum and its gradient from ONE gradient-mode
factorisation per fit) in one process, device-resident, events on one stream, median of --reps after warm-up.  fp64, N = 2048,
d = 6, SE-ARD, for 1 fit and for 64 fits:
  (a) loo_grad_ms      one cgp_loo_nll_grad_batch_device evaluation
  (b) central_ms       the route without it: 2 ntheta calls of cgp_loo_batch_device at perturbed theta (central differences)
  (c) multi_grad_ms    one cgp_multi_nll_grad_batch_device evaluation at P = 1: the marginal likelihood's gradient beside it
Prints ONE JSON line and writes it to --out (profiles/loo_opt_bench.json):
  shapes[]: fits, the three times, speedup (b / a), ratio_to_marginal (a / c), <kernel>_ms for k_loo_kinv / k_loo_grad /
            k_multi_grad (device time per launch from torch.profiler; null where the profiler does not see the library's kernels)
            and their fraction of the 78.6 TFLOP/s fp64 MFMA peak by algorithmic flops per fit (N^3 / 3, N^3, N^3 / 3 + N^2)
  optimise: one cgp_optimize_loo_batch run (N = 1024, d = 1, a slip series, from all-ones): wall ms, evaluations, lpd_sum and logml
            there, beside lpd_sum and logml at the optimum of cgp_optimize_batch on the same window
  max_err_over_bar: the timed outputs of fit 0 of the first shape against tests/loo_grad_oracle.py, after the timed regions, in
            units of the 1e-6 bar; the tool fails beyond 1"""
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fits", type=str, default="1,64")
ap.add_argument("--opt-n", type=int, default=1024)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "loo_opt_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
from corenav_gp_amd import synth
import loo_grad_oracle as lgo   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20270)
N, d, kid = args.n, 6, engine.KERNEL_SE_ARD
nth = d + 2
fits = [int(v) for v in args.fits.split(",")]
BMAX = max(fits)
KERNELS = ("k_loo_kinv", "k_loo_grad", "k_multi_grad")


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
w = rng.normal(size=(BMAX, d))
y = np.sin(np.einsum("bnd,bd->bn", X, w)) + 0.05 * rng.normal(size=(BMAX, N))
th = np.column_stack([rng.uniform(0.5, 1.5, BMAX)] + [rng.uniform(1.0, 3.0, BMAX) for _ in range(d)] + [np.full(BMAX, 0.01)])
thp = np.zeros((BMAX, engine.MAX_THETA))
thp[:, :nth] = th
f64 = dict(device=dev, dtype=torch.float64)
dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
dy, dth = torch.from_numpy(y).to(dev), torch.from_numpy(thp).to(dev)
# the 2 ntheta perturbed parameter sets of the central-difference route
H = 1e-5
dth_pm = []
for i in range(nth):
    for sgn in (1.0, -1.0):
        t = thp.copy()
        t[:, i] *= 1.0 + sgn * H
        dth_pm.append(torch.from_numpy(t).to(dev))
ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=BMAX)
ctx.loo_grad_reserve(BMAX)
ctx.multi_reserve(BMAX, 1)
ctx.multi_grad_reserve(BMAX, 1)
out = {"metric": "loo-gradient-vs-central-differences", "N": N, "d": d, "kernel": "se_ard", "peak_tflops": PEAK_TFLOPS, "shapes": []}
first = None
for B in fits:
    dn, dg, dl = torch.empty(B, **f64), torch.empty((B, nth), **f64), torch.empty(B, **f64)
    dsum = torch.empty((2 * nth, B), **f64)
    dmn, dmg, dml = torch.empty(B, **f64), torch.empty((B, nth), **f64), torch.empty((B, 1), **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)

    def run_grad():
        ctx.loo_nll_grad_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, dn.data_ptr(), dg.data_ptr(), nth,
                                      dl.data_ptr(), di.data_ptr(), stream)

    def run_central():
        for k, t in enumerate(dth_pm):
            ctx.loo_batch_device(B, N, d, kid, dX.data_ptr(), dy.data_ptr(), t.data_ptr(), 0, 0, 0, 0, dsum[k].data_ptr(), dl.data_ptr(),
                                 di.data_ptr(), stream)

    def run_multi():
        ctx.multi_nll_grad_batch_device(B, N, d, 1, kid, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, dmn.data_ptr(), dmg.data_ptr(),
                                        nth, dml.data_ptr(), di.data_ptr(), stream)

    rec = {"fits": B, "loo_grad_ms": timed(run_grad, args.reps), "central_ms": timed(run_central, args.reps, warm=1),
           "multi_grad_ms": timed(run_multi, args.reps)}
    rec["speedup"] = rec["central_ms"] / rec["loo_grad_ms"]
    rec["ratio_to_marginal"] = rec["loo_grad_ms"] / rec["multi_grad_ms"]
    run_grad()
    torch.cuda.synchronize()
    assert not di.cpu().numpy().any()
    hn, hg, hs = dn.cpu().numpy(), dg.cpu().numpy(), dsum.cpu().numpy()
    cd = np.stack([-(hs[2 * i] - hs[2 * i + 1]) / (2.0 * H * th[:B, i]) for i in range(nth)], axis=1)
    rec["routes_max_rel_diff"] = float(np.max(np.max(np.abs(hg - cd), axis=1) / np.max(np.abs(hg), axis=1)))
    k = kernel_ms(run_grad, KERNELS[:2])
    k.update(kernel_ms(run_multi, KERNELS[2:]))
    flops = {"k_loo_kinv": N ** 3 / 3.0, "k_loo_grad": float(N) ** 3, "k_multi_grad": N ** 3 / 3.0 + float(N) * N}
    for name in KERNELS:
        rec[name + "_ms"] = k[name]
        rec[name + "_frac_of_peak"] = B * flops[name] / (k[name] * 1e-3) / (PEAK_TFLOPS * 1e12) if k[name] else None
    out["shapes"].append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    if first is None:
        first = (hn.copy(), hg.copy())
# one full optimisation of a slip series on the time base, from all-ones, beside the marginal likelihood's optimum
No = args.opt_n
t = np.arange(11, 11 + No, dtype=np.float64)
yo = synth._slip_series(np.random.default_rng(9000), t)
octx = engine.Context(max_n=No, max_m=No, max_d=1, max_batch=1)
octx.loo_grad_reserve(1)
Xo = t[None, :, None]
octx.optimize_loo_batch(Xo, yo[None], kid, np.ones(3), max_evals=2)   # warm-up
t0 = time.perf_counter()
tho, lpdo, lmlo, nevo = octx.optimize_loo_batch(Xo, yo[None], kid, np.ones(3))
wall = (time.perf_counter() - t0) * 1e3
thm, lmlm, nevm = octx.optimize_batch(Xo, yo[None], kid, np.ones(3))
at_ml = octx.loo_batch(Xo, yo[None], thm, kid)
out["optimise"] = {"N": No, "d": 1, "wall_ms": wall, "evaluations": int(nevo[0]), "lpd_sum": float(lpdo[0]), "logml": float(lmlo[0]),
                   "theta": tho[0].tolist(), "logml_optimum": {"evaluations": int(nevm[0]), "lpd_sum": float(at_ml[4][0]),
                                                               "logml": float(lmlm[0]), "theta": thm[0].tolist()}}
hn, hg = first
onl, og, _, _ = lgo.nlpd_and_grad(kid, th[0], X[0], y[0])
out["max_err_over_bar"] = float(max(abs(hn[0] - onl) / abs(onl), np.max(np.abs(hg[0] - og)) / np.max(np.abs(og)))) / 1e-6
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
