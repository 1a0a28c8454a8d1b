#!/usr/bin/env python3
"""Cost of the joint forecast after a batch of fits, at the headline shape: B x (N = 2048, d = 6 SE-ARD, fp64), device-resident,
one process, the three calls ALTERNATING, events on the stream, `--warmup` calls of each then `--reps` timed calls of each:
  fit        cgp_fit_predict_batch_device alone (the marginals: what the joint calls add to)
  cov        cgp_fit_predict_cov_batch_device (fit + k_joint_cov into the caller's (B, M, M))
  sample     cgp_fit_sample_batch_device, S = 16 (fit + k_joint_cov scratch form + k_window_joint_chol + k_window_joint_paths)
for every (batch, M) of --cases.  Prints ONE JSON line; per case: median ms of each call, the added ms of the contraction
(cov - fit), its share of the 78.6 TFLOP/s fp64 MFMA peak by the flops it really ISSUES
    super-tiles of the lower triangle x 64^2 x 2 N  =  nsup (nsup + 1) / 2 x 8192 N per fit,  nsup = ceil(ceil(M / 16) / 4)
(a wave issues all sixteen tiles of a super-tile it owns except those above the diagonal of a diagonal super-tile; the useful
flops are N M^2), and the largest error of the LAST timed calls' outputs against the refit oracle on --check fits, in the metric
of tests/test_gpu_joint_batch.py::close.  Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

FP64_MFMA_PEAK_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--cases", type=str, default="512x599,64x599,512x256,512x64", help="batch x M, comma separated")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--paths", type=int, default=16)
ap.add_argument("--check", type=int, default=2, help="fits of every case compared with the oracle (0.8 s each on the host)")
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import corenav_gp_amd.synth as synth
from joint_oracle import sliding_window_joint, sample_paths   # checker only, after the timed regions
from oracle import gp_oracle as go

dev = torch.device("cuda", 0)
N, S, d = args.n, args.paths, 6
cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
Bmax, Mmax = max(b for b, _ in cases), max(m for _, m in cases)
kid, X, y, _, theta, _ = synth.config(2, batch=Bmax, N=N, M=1)
rng = np.random.default_rng(20266)
Xs_all = X[:, rng.integers(N - 50, N, size=Mmax)] + 0.3 * rng.normal(size=(Bmax, Mmax, d))   # points around the inputs
ctx = engine.Context(max_n=N, max_m=Mmax, max_d=d, max_batch=Bmax)
ctx.joint_reserve(Bmax, Mmax)
th = np.zeros((Bmax, 10))
th[:, :theta.shape[1]] = theta
stream = torch.cuda.current_stream().cuda_stream
out = {"tool": "bench_joint_batch", "N": N, "d": d, "paths": S, "reps": args.reps, "warmup": args.warmup, "cases": []}
for B, M in cases:
    Xs = np.ascontiguousarray(Xs_all[:B, :M])
    xi = rng.normal(size=(B, S, M))
    dX = torch.from_numpy(np.ascontiguousarray(X[:B].transpose(0, 2, 1))).to(dev)
    dXs = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
    dy, dth, dxi = torch.from_numpy(y[:B].copy()).to(dev), torch.from_numpy(th[:B].copy()).to(dev), torch.from_numpy(xi).to(dev)
    dm, dv = (torch.empty((B, M), dtype=torch.float64, device=dev) for _ in range(2))
    dc = torch.empty((B, M, M), dtype=torch.float64, device=dev)
    dp = torch.empty((B, S, M), dtype=torch.float64, device=dev)
    dl = torch.empty(B, dtype=torch.float64, device=dev)
    di, ds = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    head = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True)
    calls = {
        "fit": lambda: ctx.fit_predict_batch_device(*head, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(), stream),
        "cov": lambda: ctx.fit_predict_cov_batch_device(*head, dm.data_ptr(), dc.data_ptr(), dl.data_ptr(), di.data_ptr(), stream),
        "sample": lambda: ctx.fit_sample_batch_device(*head, S, dxi.data_ptr(), 1e-6, dp.data_ptr(), dl.data_ptr(), di.data_ptr(),
                                                      ds.data_ptr(), stream),
    }
    ms = {k: [] for k in calls}
    for rep in range(args.warmup + args.reps):
        for k, call in calls.items():   # alternating: every call sees the same clocks and the same neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mt = -(-M // 16)
    nsup = -(-mt // 4)
    issued = nsup * (nsup + 1) // 2 * 64 * 64 * 2.0 * N * B
    add = med["cov"] - med["fit"]
    mean, cov, paths = dm.cpu().numpy(), dc.cpu().numpy(), dp.cpu().numpy()
    assert not di.cpu().numpy().any() and not ds.cpu().numpy().any()
    err = 0.0
    for b in sorted({0, B - 1} if args.check >= 2 else ({0} if args.check else set())):
        omu, ocov = sliding_window_joint(kid, theta[b], N, X[b], y[b], Xs[b], include_noise=True)
        sd = np.sqrt(np.diag(ocov))
        sn = go.noise_var(kid, theta[b])
        op = sample_paths(omu, ocov - sn * np.eye(M), sn, 1e-6, xi[b])
        err = max(err, float(np.max(np.abs(mean[b] - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(cov[b] - ocov) / np.outer(sd, sd))),
                  float(np.max(np.abs(paths[b] - op)) / np.max(np.abs(op))))
    out["cases"].append({
        "batch": B, "M": M, "fit_ms": med["fit"], "cov_ms": med["cov"], "sample_ms": med["sample"],
        "fit_ms_min_max": [min(ms["fit"]), max(ms["fit"])], "cov_ms_min_max": [min(ms["cov"]), max(ms["cov"])],
        "sample_ms_min_max": [min(ms["sample"]), max(ms["sample"])],
        "contraction_added_ms": add, "contraction_issued_gflop": issued / 1e9, "contraction_useful_gflop": B * N * float(M) * M / 1e9,
        "contraction_frac_of_fp64_mfma_peak_by_added_ms": issued / (add * 1e-3) / (FP64_MFMA_PEAK_TFLOPS * 1e12) if add > 0 else None,
        "sample_added_ms": med["sample"] - med["fit"], "max_rel_err_vs_oracle": err, "fits_checked": args.check})
    del dc, dp
    torch.cuda.empty_cache()
print(json.dumps(out))
