#!/usr/bin/env python3
"""Benchmark of the sparse fits with P target columns against the single-column call, in one process (one box, one clock state), by
tools/bench_sparse.py's method: fp64, SE-iso, d = 1 tick histories, 64 fits, device-resident, M test points.

  per shape (N, m) in (2048, 256), (65536, 256), (65536, 512) and P in 1, 4, 16:
    multi_ms     host clock around cgp_fit_predict_sparse_multi_batch_device + a synchronisation, median of --reps after warm-up
    single_ms    the same around cgp_fit_predict_sparse_batch_device on column 0: the reference, what a caller pays per column today
    r            multi_ms / (P single_ms): the share of P single-column calls that the shared fit costs
    kernels_ms   per-kernel time of one multi call via cgp_profile_* (events around every launch): phi, reduce, algebra, predict, prep
    single_kernels_ms   the same of the single-column call
Prints ONE JSON line and writes it to --out (profiles/sparse_multi_bench.json).  gate: r at P = 4 and k_sparse_phi's time at P = 4
over P = 1 at (65536, 256), when that shape is among --shapes.  max_err_over_bar: the timed outputs of fit 0 of the first shape and
column count against tests/sparse_multi_oracle.py in units of the 1e-6 bar; columns_bitwise_single: column 0 of every multi call
against the single-column call's outputs.  The tool fails beyond the bar or on a column that is not bitwise."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, default="2048x256,65536x256,65536x512")
ap.add_argument("--columns", type=str, default="1,4,16")
ap.add_argument("--fits", type=int, default=64)
ap.add_argument("--m", type=int, default=599)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sparse_multi_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import sparse_multi_oracle as smo   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20282)
B, M, kid, d = args.fits, args.m, engine.KERNEL_SE_ISO, 1
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
PS = [int(v) for v in args.columns.split(",")]
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


def profiled(ctx, call):
    ctx.profile_enable(True)
    ctx.profile_read()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {NAMES[i]: prof[engine.PROF_NAMES[i]]["ms"] / 3.0 for i in NAMES}


def histories(N, m, P):
    """bench_sparse.py's tick histories with P target columns: a phase per fit and column."""
    t = np.arange(N, dtype=np.float64)[None] + rng.integers(0, 50, size=(B, 1))
    ell = (N - 1) / ((m - 1) * 1.25)
    ph = rng.uniform(0, 6.0, size=(B, P, 1))
    Y = 0.1 * np.sin(t[:, None] / ell * 0.9 + ph) + 0.05 * np.cos(t[:, None] / ell * 0.31 + 1.0) + np.sqrt(1e-3) * rng.normal(size=(B, P, N))
    Z = np.linspace(t[:, 0], t[:, -1], m, axis=1)
    Xs = t[:, :1] + (N - 1.0) * rng.random((B, M))
    theta = np.tile([0.02, ell, 1e-3], (B, 1))
    return t[:, :, None], Y, Z[:, :, None], Xs[:, :, None], theta


out = {"metric": "sparse-multi-fit-predict", "fits": B, "M": M, "d": d, "kernel": "se_iso", "shapes": []}
worst, bitwise = None, True
for N, m in SHAPES:
    Pmax = max(PS)
    X, Y, Z, Xs, theta = histories(N, m, Pmax)
    thp = np.zeros((B, engine.MAX_THETA))
    thp[:, :3] = theta
    dX, dZ, dXs, dth = up(X.transpose(0, 2, 1)), up(Z.transpose(0, 2, 1)), up(Xs.transpose(0, 2, 1)), up(thp)
    ctx = engine.Context(max_n=128, max_m=M, max_d=d, max_batch=B)
    ctx.sparse_reserve(B, N, m, M)
    ctx.sparse_multi_reserve(B, Pmax)
    di = torch.zeros(B, device=dev, dtype=torch.int32)
    dy = up(Y[:, 0])
    sm, sv, sl = torch.empty((B, M), **f64), torch.empty((B, M), **f64), torch.empty(B, **f64)

    def run_single():
        ctx.fit_predict_sparse_batch_device(B, N, d, M, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dXs.data_ptr(), dth.data_ptr(),
                                            0, True, sm.data_ptr(), sv.data_ptr(), sl.data_ptr(), di.data_ptr(), stream)

    single = timed(run_single, args.reps)
    assert not di.cpu().numpy().any()
    rec = {"N": N, "m": m, "single_ms": single[0], "single_ms_min": single[1], "single_ms_max": single[2],
           "single_kernels_ms": profiled(ctx, run_single), "columns": []}
    for P in PS:
        dY = up(Y[:, :P])
        dm, dv, dl = torch.empty((B, P, M), **f64), torch.empty((B, M), **f64), torch.empty((B, P), **f64)

        def run_multi():
            ctx.fit_predict_sparse_multi_batch_device(B, N, d, M, P, m, kid, dX.data_ptr(), dY.data_ptr(), dZ.data_ptr(), dXs.data_ptr(),
                                                      dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(),
                                                      stream)

        med, lo, hi = timed(run_multi, args.reps)
        assert not di.cpu().numpy().any()
        bitwise = bitwise and bool(torch.equal(dm[:, 0], sm) and torch.equal(dv, sv) and torch.equal(dl[:, 0], sl))
        if worst is None:
            o = smo.one_factor(kid, theta[0], X[0], Y[0, :P], Z[0], Xs[0])
            worst = max(smo.errors(dm[0].cpu().numpy(), dv[0].cpu().numpy(), dl[0].cpu().numpy(), o)) / 1e-6
        rec["columns"].append({"P": P, "multi_ms": med, "multi_ms_min": lo, "multi_ms_max": hi, "r": med / (P * single[0]),
                               "kernels_ms": profiled(ctx, run_multi)})
        del dY, dm, dv, dl
    out["shapes"].append(rec)
    ctx.close()
    del dX, dy, dZ, dXs
for rec in out["shapes"]:
    if (rec["N"], rec["m"]) == (65536, 256):
        by = {c["P"]: c for c in rec["columns"]}
        if 1 in by and 4 in by:
            out["gate"] = {"r_4": by[4]["r"], "r_4_bar": 0.5, "phi_p4_over_p1": by[4]["kernels_ms"]["phi"] / by[1]["kernels_ms"]["phi"],
                           "phi_bar": 1.1}
            out["gate"]["met"] = bool(out["gate"]["r_4"] <= 0.5 and out["gate"]["phi_p4_over_p1"] <= 1.1)
out["max_err_over_bar"] = float(worst)
out["columns_bitwise_single"] = bitwise
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 and bitwise else 1)
