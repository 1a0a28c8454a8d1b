#!/usr/bin/env python3
"""Benchmark of the predictive gradients beside the marginal call they extend, in one process on the same samples (same-process
A/B: one box, one clock state).  fp64, N = 2048, d = 6, SE-ARD, device-resident; the two calls alternate, device events around each
on one stream after warm-up, medians of --reps (>= 20).  Prints ONE JSON line and writes it to --out (profiles/pgrad_bench.json):
  shapes[]: fits, M, fit_ms (cgp_fit_predict_batch_device), grad_ms (cgp_fit_predict_grad_batch_device), added_ms, added_frac,
            k_pgrad_solve_ms, k_pgrad_contract_ms and, for the same fits and N, k_multi_solve_ms at P = M + 1 -- existing code
            doing the same flop count in the forward direction, the yardstick -- (device time per launch from torch.profiler;
            null where the profiler does not see the library's kernels), solve_ratio = k_pgrad_solve / k_multi_solve, the
            solves' fraction of the 78.6 TFLOP/s fp64 MFMA peak by algorithmic flops (N^2 (M + 1) per fit), and the
            contraction's entries (N M per fit) per second
  max_err_over_bar: the timed gradients of the last shape's fit 0 against tests/pgrad_oracle.py, after the timed regions, in units
            of the 1e-6 bar; the tool fails beyond 1"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", type=str, default="512x599,64x599,512x64")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pgrad_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import pgrad_oracle as po   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20269)
N, d, kid = args.n, 6, engine.KERNEL_SE_ARD
shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
BMAX, MMAX = max(b for b, _ in shapes), max(m for _, m in shapes)


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
Xs = rng.uniform(-2.0, 2.0, (BMAX, MMAX, d))
w = rng.normal(size=(BMAX, d))
y = np.sin(np.einsum("bnd,bd->bn", X, w)) + 0.05 * rng.normal(size=(BMAX, N))
th = np.column_stack([rng.uniform(0.5, 1.5, BMAX)] + [rng.uniform(1.0, 3.0, BMAX) for _ in range(d)] + [np.full(BMAX, 0.01)])
thp = np.zeros((BMAX, engine.MAX_THETA))
thp[:, :d + 2] = th
f64 = dict(device=dev, dtype=torch.float64)
dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
dy, dth = torch.from_numpy(y).to(dev), torch.from_numpy(thp).to(dev)
ctx = engine.Context(max_n=N, max_m=MMAX, max_d=d, max_batch=BMAX)
assert ctx.pgrad_reserve(BMAX, MMAX) == 0
assert ctx.multi_reserve(BMAX, MMAX + 1) == 0
out = {"metric": "predictive-gradients-vs-marginal-call", "N": N, "d": d, "kernel": "se_ard", "peak_tflops": PEAK_TFLOPS,
       "reps": args.reps, "shapes": []}
last = None
for B, M in shapes:
    dXs = torch.from_numpy(np.ascontiguousarray(Xs[:B, :M].transpose(0, 2, 1))).to(dev)
    dm, dv, dl = torch.empty((B, M), **f64), torch.empty((B, M), **f64), torch.empty(B, **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)
    gm, gv = torch.empty((B, M, d), **f64), torch.empty((B, M, d), **f64)
    base = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(),
            dl.data_ptr(), di.data_ptr())

    def run_fit():
        ctx.fit_predict_batch_device(*base, stream)

    def run_grad():
        ctx.fit_predict_grad_batch_device(*base, gm.data_ptr(), gv.data_ptr(), stream)

    for _ in range(2):
        run_fit()
        run_grad()
    torch.cuda.synchronize()
    ms = {"fit": [], "grad": []}
    for _ in range(args.reps):
        for name, call in (("fit", run_fit), ("grad", run_grad)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    assert not di.cpu().numpy().any()
    rec = {"fits": B, "M": M, "fit_ms": float(np.median(ms["fit"])), "grad_ms": float(np.median(ms["grad"]))}
    rec["added_ms"] = rec["grad_ms"] - rec["fit_ms"]
    rec["added_frac"] = rec["added_ms"] / rec["fit_ms"]
    k = kernel_ms(run_grad, ("k_pgrad_solve", "k_pgrad_contract"))
    # the yardstick: the forward multi-right-hand-side solve of the same fits with P = M + 1 targets
    P = M + 1
    dY = torch.from_numpy(rng.normal(size=(B, P, N))).to(dev)
    mm, ml = torch.empty((B, P, M), **f64), torch.empty((B, P), **f64)

    def run_multi():
        ctx.fit_predict_multi_batch_device(B, N, d, M, P, kid, dX.data_ptr(), dY.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                           mm.data_ptr(), dv.data_ptr(), ml.data_ptr(), di.data_ptr(), stream)

    run_multi()
    torch.cuda.synchronize()
    k.update(kernel_ms(run_multi, ("k_multi_solve",)))
    flops = float(B) * N * N * P
    for name in ("k_pgrad_solve", "k_multi_solve"):
        rec[name + "_ms"] = k[name]
        rec[name + "_frac_of_peak"] = flops / (k[name] * 1e-3) / (PEAK_TFLOPS * 1e12) if k[name] else None
    rec["solve_ratio"] = k["k_pgrad_solve"] / k["k_multi_solve"] if k["k_pgrad_solve"] and k["k_multi_solve"] else None
    rec["k_pgrad_contract_ms"] = k["k_pgrad_contract"]
    rec["contract_entries_per_s"] = float(B) * N * M / (k["k_pgrad_contract"] * 1e-3) if k["k_pgrad_contract"] else None
    out["shapes"].append(rec)
    run_grad()
    torch.cuda.synchronize()
    last = (M, gm[0].cpu().numpy(), gv[0].cpu().numpy())
    del dY, mm, ml
M, gdm, gdv = last
odm, odv = po.predictive_gradients(po.fit(kid, th[0], X[0], y[0]), Xs[0, :M])
out["max_err_over_bar"] = float(max(np.max(np.abs(gdm - odm)) / np.max(np.abs(odm)), np.max(np.abs(gdv - odv)) / np.max(np.abs(odv)))) / 1e-6
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
