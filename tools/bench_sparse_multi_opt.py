#!/usr/bin/env python3
"""Benchmark of the sparse fits' objective with P target columns, in one process (one box, one clock state),
tools/bench_sparse_opt.py's method: fp64, SE-iso, d = 1 tick histories, 64 fits, device-resident, dgradZ asked.

  per shape (N, m) in (2048, 256), (16384, 256), (65536, 256), (65536, 512):
    single_ms    host clock around cgp_sparse_nll_grad_batch_device + a synchronisation, median of --reps after warm-up, with the
                 min and max of the reps: this build's single-column call
    per P in 1, 4, 16:
      ms         the same around cgp_sparse_multi_nll_grad_batch_device (dlogml asked)
      kernels_ms per-slot time of one such call via cgp_profile_*: phi, algebra (both algebra kernels), tail (reduce + uu +
                 finish), panel (k_sparse_grad_panel), prep
      r_single   ms / (P x single_ms): against P single-column calls of this build
  --parent FILE: the JSON that the PARENT commit's tools/bench_sparse_opt.py wrote on the same machine in the same job (its
  library built from a checkout of that commit): the yardstick.  Per shape the record then also holds parent_grad_z_ms (median,
  min, max), parent_panel_ms, r_P = ms / (P x parent_grad_z_ms) and panel_over_parent per P, and `conditions`:
    1  r_4 <= 0.5 at (65536, 256)
    2  k_sparse_grad_panel at P = 4 <= 1.1 x the parent's panel time, per shape
    3  single_ms within the parent's [min, max] widened by that range's width on either side, per shape
  reported, not enforced: the tool fails only when the timed outputs are wrong.
Prints ONE JSON line and writes it to --out (profiles/sparse_multi_grad_bench.json).  max_err_over_bar: the timed outputs of fit 0
of the first shape at the largest P against tests/sparse_multi_grad_oracle.py in units of the 1e-6 bar; the tool fails beyond 1."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, default="2048x256,16384x256,65536x256,65536x512")
ap.add_argument("--columns", type=str, default="1,4,16")
ap.add_argument("--fits", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--parent", type=str, default="")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sparse_multi_grad_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import sparse_multi_grad_oracle as smg   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20291)
B, kid, d = args.fits, engine.KERNEL_SE_ISO, 1
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
PS = [int(v) for v in args.columns.split(",")]
f64 = dict(device=dev, dtype=torch.float64)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
NAMES = {0: "phi", 1: "algebra", 2: "tail", 3: "panel", 4: "prep"}
parent = {(r["N"], r["m"]): r for r in json.load(open(args.parent))["shapes"]} if args.parent else {}


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


def histories(N, m, P):
    """tools/bench_sparse_opt.py's histories (the same generator state: column 0 is its y) with P - 1 further columns."""
    t = np.arange(N, dtype=np.float64)[None] + rng.integers(0, 50, size=(B, 1))
    ell = (N - 1) / ((m - 1) * 1.25)
    ph = rng.uniform(0, 6.0, size=(B, 1))
    y = 0.1 * np.sin(t / ell * 0.9 + ph) + 0.05 * np.cos(t / ell * 0.31 + 1.0) + np.sqrt(1e-3) * rng.normal(size=(B, N))
    Z = np.linspace(t[:, 0], t[:, -1], m, axis=1)
    theta = np.tile([0.02, ell, 1e-3], (B, 1))
    rest = np.random.default_rng(977 + N + m)
    Y = np.empty((B, P, N))
    Y[:, 0] = y
    for p in range(1, P):
        Y[:, p] = 0.1 * np.sin(t / ell * 0.9 + ph + 0.7 * p) + 0.05 * np.cos(t / ell * 0.31 + p) + np.sqrt(1e-3) * rest.normal(size=(B, N))
    return t[:, :, None], Y, Z[:, :, None], theta


out = {"metric": "sparse-multi-nll-grad", "fits": B, "d": d, "kernel": "se_iso", "grad_z": 1, "columns": PS, "shapes": [],
       "parent": bool(parent)}
worst = None
for N, m in SHAPES:
    Pmax = max(PS)
    X, Y, Z, theta = histories(N, m, Pmax)
    thp = np.zeros((B, engine.MAX_THETA))
    thp[:, :3] = theta
    dX, dY, dZ, dth = up(X.transpose(0, 2, 1)), up(Y), up(Z.transpose(0, 2, 1)), up(thp)
    dy = dY[:, 0].contiguous()
    dn, dg, dgz = torch.empty(B, **f64), torch.empty((B, engine.MAX_THETA), **f64), torch.empty((B, d, m), **f64)
    di = torch.zeros(B, device=dev, dtype=torch.int32)
    ctx = engine.Context(max_n=128, max_m=8, max_d=d, max_batch=B)
    ctx.sparse_reserve(B, N, m, 0)
    ctx.sparse_grad_reserve(B)
    ctx.sparse_multi_reserve(B, Pmax)
    ctx.sparse_multi_grad_reserve(B, Pmax)

    def run_single():
        ctx.sparse_nll_grad_batch_device(B, N, d, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0, dn.data_ptr(),
                                         dg.data_ptr(), engine.MAX_THETA, dgz.data_ptr(), di.data_ptr(), stream)

    def run_multi(dYp, dl, P):
        ctx.sparse_multi_nll_grad_batch_device(B, N, d, P, m, kid, dX.data_ptr(), dYp.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0,
                                               dn.data_ptr(), dg.data_ptr(), engine.MAX_THETA, dgz.data_ptr(), dl.data_ptr(),
                                               di.data_ptr(), stream)

    rec = {"N": N, "m": m, "columns": []}
    rec["single_ms"], rec["single_ms_min"], rec["single_ms_max"] = timed(run_single, args.reps)
    par = parent.get((N, m))
    if par:
        lo, hi = par["grad_z_ms_min"], par["grad_z_ms_max"]
        rec["parent_grad_z_ms"], rec["parent_grad_z_ms_min"], rec["parent_grad_z_ms_max"] = par["grad_z_ms"], lo, hi
        rec["parent_panel_ms"] = par["kernels_ms"]["panel"]
        rec["single_within_parent_range"] = bool(lo - (hi - lo) <= rec["single_ms"] <= hi + (hi - lo))
    for P in PS:
        dYp = dY[:, :P].contiguous()
        dl = torch.empty((B, P), **f64)
        col = {"P": P}
        col["ms"], col["ms_min"], col["ms_max"] = timed(lambda: run_multi(dYp, dl, P), args.reps)
        assert not di.cpu().numpy().any()
        col["r_single"] = col["ms"] / (P * rec["single_ms"])
        if worst is None and P == Pmax:
            onll, og, ogz, ologml, info = smg.one_factor(kid, theta[0], X[0], Y[0, :P], Z[0])
            e = [abs(float(dn[0].cpu()) - onll) / max(1.0, abs(onll)), np.max(np.abs(dg[0, :3].cpu().numpy() - og)) / np.max(np.abs(og)),
                 np.max(np.abs(dgz[0].cpu().numpy().T - ogz)) / np.max(np.abs(ogz)),
                 np.max(np.abs(dl[0].cpu().numpy() - ologml) / np.maximum(1.0, np.abs(ologml)))]
            worst = float(max(e)) / 1e-6
        ctx.profile_enable(True)
        ctx.profile_read()
        for _ in range(3):
            run_multi(dYp, dl, P)
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        col["kernels_ms"] = {NAMES[i]: prof[engine.PROF_NAMES[i]]["ms"] / 3.0 for i in NAMES}
        if par:
            col["r_parent"] = col["ms"] / (P * par["grad_z_ms"])
            col["panel_over_parent"] = col["kernels_ms"]["panel"] / par["kernels_ms"]["panel"]
        rec["columns"].append(col)
        del dYp, dl
    out["shapes"].append(rec)
    ctx.close()
    del dX, dY, dy, dZ, dgz
if parent:
    by = {(r["N"], r["m"]): r for r in out["shapes"]}
    col = lambda r, P: next((c for c in r["columns"] if c["P"] == P), None)
    r4 = col(by[(65536, 256)], 4) if (65536, 256) in by else None
    out["conditions"] = {
        "1_r4_at_65536x256": None if r4 is None else {"r_4": r4["r_parent"], "bar": 0.5, "met": bool(r4["r_parent"] <= 0.5)},
        "2_panel_p4_over_parent": {f"{r['N']}x{r['m']}": {"ratio": col(r, 4)["panel_over_parent"], "bar": 1.1,
                                                        "met": bool(col(r, 4)["panel_over_parent"] <= 1.1)}
                                   for r in out["shapes"] if col(r, 4) and "parent_panel_ms" in r},
        "3_single_within_parent_range": {f"{r['N']}x{r['m']}": r["single_within_parent_range"] for r in out["shapes"]
                                         if "single_within_parent_range" in r}}
out["max_err_over_bar"] = float(worst)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
