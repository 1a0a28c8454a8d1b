#!/usr/bin/env python3
"""Benchmark of the sparse fits' objective, in one process (one box, one clock state), tools/bench_sparse.py's method: fp64,
SE-iso, d = 1 tick histories, 64 fits, device-resident.

  per shape (N, m) in (2048, 256), (16384, 256), (65536, 256), (65536, 512):
    forward_ms   host clock around cgp_fit_predict_sparse_batch_device at M = 0 + a synchronisation, median of --reps after warm-up:
                 the yardstick, measured beside the two below in the same run
    grad_ms, grad_z_ms   the same around cgp_sparse_nll_grad_batch_device without and with dgradZ; *_over_forward their ratios
    kernels_ms   per-slot time of one gradient call (with dgradZ) via cgp_profile_*: phi, algebra (both algebra kernels), tail
                 (reduce + uu + finish), panel (k_sparse_grad_panel), prep
    panel_tflops, panel_of_peak   k_sparse_grad_panel's recorded flops 2 N (m + 1) LD per fit over its time, against the 78.6 TFLOP/s
                 fp64 MFMA peak
  optimiser: one cgp_optimize_sparse_batch run with optimize_z = 1 (--opt-fits fits of the first shape, --opt-evals evaluations at
  most): evaluations and wall time.
Prints ONE JSON line and writes it to --out (profiles/sparse_grad_bench.json).  max_err_over_bar: the timed outputs of fit 0 of the
first shape against tests/sparse_grad_oracle.py in units of the 1e-6 bar; the tool fails beyond 1."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, default="2048x256,16384x256,65536x256,65536x512")
ap.add_argument("--fits", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--opt-fits", type=int, default=4)
ap.add_argument("--opt-evals", type=int, default=60)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sparse_grad_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import sparse_grad_oracle as sg   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20291)
PEAK = 78.6e12
B, kid, d = args.fits, engine.KERNEL_SE_ISO, 1
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
f64 = dict(device=dev, dtype=torch.float64)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
NAMES = {0: "phi", 1: "algebra", 2: "tail", 3: "panel", 4: "prep"}


def timed(call, n):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def histories(N, m):
    """B tick histories of N samples, m inducing inputs spread over each at 1.25 length-scales (tools/bench_sparse.py's)."""
    t = np.arange(N, dtype=np.float64)[None] + rng.integers(0, 50, size=(B, 1))
    ell = (N - 1) / ((m - 1) * 1.25)
    ph = rng.uniform(0, 6.0, size=(B, 1))
    y = 0.1 * np.sin(t / ell * 0.9 + ph) + 0.05 * np.cos(t / ell * 0.31 + 1.0) + np.sqrt(1e-3) * rng.normal(size=(B, N))
    Z = np.linspace(t[:, 0], t[:, -1], m, axis=1)
    theta = np.tile([0.02, ell, 1e-3], (B, 1))
    return t[:, :, None], y, Z[:, :, None], theta


out = {"metric": "sparse-nll-grad", "fits": B, "d": d, "kernel": "se_iso", "peak_tflops_fp64_mfma": PEAK / 1e12, "shapes": []}
worst = None
for N, m in SHAPES:
    X, y, Z, theta = histories(N, m)
    thp = np.zeros((B, engine.MAX_THETA))
    thp[:, :3] = theta
    dX, dy, dZ, dth = up(X.transpose(0, 2, 1)), up(y), up(Z.transpose(0, 2, 1)), up(thp)
    dn, dg, dgz, dl = torch.empty(B, **f64), torch.empty((B, engine.MAX_THETA), **f64), torch.empty((B, d, m), **f64), torch.empty(B, **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)
    ctx = engine.Context(max_n=128, max_m=8, max_d=d, max_batch=B)
    ctx.sparse_reserve(B, N, m, 0)
    ctx.sparse_grad_reserve(B)

    def run_forward():
        ctx.fit_predict_sparse_batch_device(B, N, d, 0, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), 0, dth.data_ptr(), 0, True, 0, 0,
                                            dl.data_ptr(), di.data_ptr(), stream)

    def run_grad(with_z):
        ctx.sparse_nll_grad_batch_device(B, N, d, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0, dn.data_ptr(),
                                         dg.data_ptr(), engine.MAX_THETA, dgz.data_ptr() if with_z else 0, di.data_ptr(), stream)

    rec = {"N": N, "m": m}
    rec["forward_ms"], rec["forward_ms_min"], rec["forward_ms_max"] = timed(run_forward, args.reps)
    rec["grad_ms"], rec["grad_ms_min"], rec["grad_ms_max"] = timed(lambda: run_grad(False), args.reps)
    rec["grad_z_ms"], rec["grad_z_ms_min"], rec["grad_z_ms_max"] = timed(lambda: run_grad(True), args.reps)
    assert not di.cpu().numpy().any()
    rec["grad_over_forward"] = rec["grad_ms"] / rec["forward_ms"]
    rec["grad_z_over_forward"] = rec["grad_z_ms"] / rec["forward_ms"]
    if worst is None:
        onll, og, ogz, info = sg.nll_grad(kid, theta[0], X[0], y[0], Z[0])
        e = [abs(float(dn[0].cpu()) - onll) / max(1.0, abs(onll)), np.max(np.abs(dg[0, :3].cpu().numpy() - og)) / np.max(np.abs(og)),
             np.max(np.abs(dgz[0].cpu().numpy().T - ogz)) / np.max(np.abs(ogz))]
        worst = float(max(e)) / 1e-6
    ctx.profile_enable(True)
    ctx.profile_read()
    for _ in range(3):
        run_grad(True)
    torch.cuda.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    per = {NAMES[i]: prof[engine.PROF_NAMES[i]]["ms"] / 3.0 for i in NAMES}
    rec["kernels_ms"] = per
    LD = (m + 1 + 15) // 16 * 16
    rec["panel_tflops"] = B * 2.0 * N * (m + 1) * LD / (per["panel"] * 1e-3) / 1e12
    rec["panel_of_peak"] = rec["panel_tflops"] * 1e12 / PEAK
    out["shapes"].append(rec)
    if "optimiser" not in out:
        nb = min(args.opt_fits, B)
        t0 = time.perf_counter()
        th, Zr, bound, nev = ctx.optimize_sparse_batch(X[:nb], y[:nb], Z[:nb], theta[:nb], kid, optimize_z=True, max_evals=args.opt_evals)
        out["optimiser"] = {"N": N, "m": m, "fits": nb, "optimize_z": 1, "max_evals": args.opt_evals, "evaluations": [int(v) for v in nev],
                            "wall_s": time.perf_counter() - t0, "bound_fit0": float(bound[0])}
    ctx.close()
    del dX, dy, dZ, dgz
out["max_err_over_bar"] = float(worst)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
