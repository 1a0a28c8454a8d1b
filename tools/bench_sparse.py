#!/usr/bin/env python3
"""Benchmark of the sparse (inducing-point) fits, in one process (one box, one clock state): fp64, SE-iso, d = 1 tick histories,
64 fits, device-resident, M test points.

  per shape (N, m) in (2048, 256), (16384, 256), (65536, 256), (65536, 512):
    call_ms      host clock around cgp_fit_predict_sparse_batch_device + a synchronisation, median of --reps after warm-up
    kernels      per-kernel time of one call via cgp_profile_* (events around every launch): phi, reduce, algebra, predict, prep
    phi_tflops, phi_of_peak   k_sparse_phi's algorithmic flops N (m + 1)(m + 2) per fit over its time, against the 78.6 TFLOP/s
                 fp64 MFMA peak
  at N = 2048: dense_ms, cgp_fit_predict_batch_device on the same samples and test points -- the reference for "is the sparse
  route worth taking at this size" -- and sparse_over_dense.
Prints ONE JSON line and writes it to --out (profiles/sparse_bench.json).  max_err_over_bar: the timed outputs of fit 0 of the first
shape against tests/sparse_oracle.py in units of the 1e-6 bar; the tool fails beyond 1."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, default="2048x256,16384x256,65536x256,65536x512")
ap.add_argument("--fits", type=int, default=64)
ap.add_argument("--m", type=int, default=599)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sparse_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import sparse_oracle as so   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20281)
PEAK = 78.6e12
B, M, kid, d = args.fits, args.m, engine.KERNEL_SE_ISO, 1
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
f64 = dict(device=dev, dtype=torch.float64)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
NAMES = {0: "phi", 1: "algebra", 2: "reduce", 3: "predict", 4: "prep"}


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
    """B tick histories of N samples, m inducing inputs spread over each at 1.25 length-scales, M test points inside."""
    t = np.arange(N, dtype=np.float64)[None] + rng.integers(0, 50, size=(B, 1))
    ell = (N - 1) / ((m - 1) * 1.25)
    ph = rng.uniform(0, 6.0, size=(B, 1))
    y = 0.1 * np.sin(t / ell * 0.9 + ph) + 0.05 * np.cos(t / ell * 0.31 + 1.0) + np.sqrt(1e-3) * rng.normal(size=(B, N))
    Z = np.linspace(t[:, 0], t[:, -1], m, axis=1)
    Xs = t[:, :1] + (N - 1.0) * rng.random((B, M))
    theta = np.tile([0.02, ell, 1e-3], (B, 1))
    return t[:, :, None], y, Z[:, :, None], Xs[:, :, None], theta


out = {"metric": "sparse-fit-predict", "fits": B, "M": M, "d": d, "kernel": "se_iso", "peak_tflops_fp64_mfma": PEAK / 1e12, "shapes": []}
worst = None
for N, m in SHAPES:
    X, y, Z, Xs, theta = histories(N, m)
    thp = np.zeros((B, engine.MAX_THETA))
    thp[:, :3] = theta
    dX, dy, dZ, dXs, dth = up(X.transpose(0, 2, 1)), up(y), up(Z.transpose(0, 2, 1)), up(Xs.transpose(0, 2, 1)), up(thp)
    dm, dv, dl = torch.empty((B, M), **f64), torch.empty((B, M), **f64), torch.empty(B, **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)
    dense = N <= 2048
    ctx = engine.Context(max_n=N if dense else 128, max_m=M, max_d=d, max_batch=B)
    ctx.sparse_reserve(B, N, m, M)

    def run_sparse():
        ctx.fit_predict_sparse_batch_device(B, N, d, M, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dXs.data_ptr(), dth.data_ptr(),
                                            0, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(), stream)

    med, lo, hi = timed(run_sparse, args.reps)
    assert not di.cpu().numpy().any()
    rec = {"N": N, "m": m, "call_ms": med, "call_ms_min": lo, "call_ms_max": hi}
    if worst is None:
        o = so.fit_predict_sparse(kid, theta[0], X[0], y[0], Z[0], Xs[0])
        assert so.conditions_hold(o), (o.ladder, o.cond_uu, o.cond_b)
        worst = max(so.errors(dm[0].cpu().numpy(), dv[0].cpu().numpy(), float(dl[0].cpu()), o)) / 1e-6
    ctx.profile_enable(True)
    ctx.profile_read()
    for _ in range(3):
        run_sparse()
    torch.cuda.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    per = {NAMES[i]: prof[engine.PROF_NAMES[i]]["ms"] / 3.0 for i in NAMES}
    rec["kernels_ms"] = per
    flops = B * float(N) * (m + 1) * (m + 2)
    rec["phi_tflops"] = flops / (per["phi"] * 1e-3) / 1e12
    rec["phi_of_peak"] = rec["phi_tflops"] * 1e12 / PEAK
    if dense:
        em, ev, el = torch.empty((B, M), **f64), torch.empty((B, M), **f64), torch.empty(B, **f64)

        def run_dense():
            ctx.fit_predict_batch_device(B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                         em.data_ptr(), ev.data_ptr(), el.data_ptr(), di.data_ptr(), stream)

        rec["dense_ms"], rec["dense_ms_min"], rec["dense_ms_max"] = timed(run_dense, args.reps)
        assert not di.cpu().numpy().any()
        rec["sparse_over_dense"] = rec["call_ms"] / rec["dense_ms"]
        rec["bound_minus_dense_logml_fit0"] = float(dl[0].cpu() - el[0].cpu())
    out["shapes"].append(rec)
    ctx.close()
    del dX, dy, dZ, dXs, dm, dv
out["max_err_over_bar"] = float(worst)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
