#!/usr/bin/env python3
"""Benchmark of the Matern kernels beside SE_ARD: the same samples, the same theta layout, the same process, alternating calls
(same-process A/B: one box, one clock state).  fp64, device-resident, events on the stream.  Prints ONE JSON line; per kernel
K in (se_ard, matern32, matern52):
  full_ms_K, full_fits_per_s_K      cgp_fit_predict_batch_device, `--full` fits x N = 2048, d = 6, M = 599 (the headline workload's shape)
  mid_ms_K                          the same call at `--mid` fits x N = 1024 (the mid-size schedule)
  push_us_per_tick_K                `--windows` windows x N = 512, d = 3: one steady-state tick of cgp_window_push_device (blocks of 64)
  forecast_ms_K                     cgp_window_predict_device, M = 599 on those windows
  node_ms_K, node_opt_ms_K          one 134-sample d = 1 window with 599 test points, host buffers: cgp_slip_node_callback at fixed
                                    theta and cgp_slip_node_callback_opt from all-ones (se_ard: the one-launch short-window kernels;
                                    Matern: tiled schedules and the host optimiser over device gradients), node_opt_evals_K
  full_matern52_over_se_ard, ...    the ratios of the times
  max_rel_err_vs_oracle             the timed Matern outputs against tests/matern_oracle.py (two fits / two windows per
                                    workload), after the timed regions; the tool fails beyond 1e-6"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--full", type=int, default=512)
ap.add_argument("--mid", type=int, default=64)
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ticks", type=int, default=128)
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import corenav_gp_amd.synth as synth
import matern_oracle as mo   # checker only, after the timed regions
from oracle import gp_oracle as go
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
KERNELS = (("se_ard", engine.KERNEL_SE_ARD), ("matern32", engine.KERNEL_MATERN32_ARD), ("matern52", engine.KERNEL_MATERN52_ARD))
M = 599
rng = np.random.default_rng(20266)
out = {"metric": "matern-vs-se_ard", "full_fits": args.full, "mid_fits": args.mid, "windows": args.windows, "M": M}
err = 0.0


def timed(calls, n):
    """Interleaved timing of several calls: per repetition every call once, in turn; returns the median ms of each."""
    for c in calls:
        c()
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for _ in range(n):
        for i, c in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [float(np.median(m)) for m in ms]


def oracle_fit(kid, th, X, y):
    return go.fit(kid, th, X, y) if kid == engine.KERNEL_SE_ARD else mo.fit(kid, th, X, y)


def oracle_predict(kid, f, Xs):
    return go.predict(f, Xs) if kid == engine.KERNEL_SE_ARD else mo.predict(f, Xs)


# ---- batched fit + predict: full batch and mid-size -------------------------------------------------------------------------------
def batch_case(tag, B, N, d):
    global err
    X = rng.uniform(-2.0, 2.0, (B, N, d))
    w = rng.normal(size=(B, d, 1))
    y = np.sin(X @ w)[:, :, 0] + 0.05 * rng.normal(size=(B, N))
    Xs = rng.uniform(-2.0, 2.0, (B, M, d))
    th = np.column_stack([rng.uniform(0.5, 1.5, B)] + [rng.uniform(1.0, 3.0, B) for _ in range(d)] + [np.full(B, 0.01)])
    thp = np.zeros((B, engine.MAX_THETA))
    thp[:, :d + 2] = th
    dX = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)
    dXs = torch.from_numpy(np.ascontiguousarray(Xs.transpose(0, 2, 1))).to(dev)
    dy, dth = torch.from_numpy(y).to(dev), torch.from_numpy(thp).to(dev)
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    res = {}
    for name, kid in KERNELS:
        res[name] = (torch.empty((B, M), device=dev, dtype=torch.float64), torch.empty((B, M), device=dev, dtype=torch.float64),
                     torch.empty(B, device=dev, dtype=torch.float64), torch.zeros(B, device=dev, dtype=torch.int32))

    def call(name, kid):
        m, v, l, i = res[name]
        return lambda: ctx.fit_predict_batch_device(B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                                    m.data_ptr(), v.data_ptr(), l.data_ptr(), i.data_ptr(), stream)
    ms = timed([call(n, k) for n, k in KERNELS], args.reps)
    for (name, kid), t in zip(KERNELS, ms):
        out[f"{tag}_ms_{name}"] = t
        if tag == "full":
            out[f"full_fits_per_s_{name}"] = B / (t * 1e-3)
        m, v, l, i = (a.cpu().numpy() for a in res[name])
        assert not i.any()
        for b in sorted({0, B - 1}):
            f = oracle_fit(kid, th[b], X[b], y[b])
            omu, ovar = oracle_predict(kid, f, Xs[b])
            err = max(err, float(np.max(np.abs(m[b] - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(v[b] - ovar) / ovar)),
                      abs(l[b] - f.logml) / abs(f.logml))
    for name in ("matern32", "matern52"):
        out[f"{tag}_{name}_over_se_ard"] = out[f"{tag}_ms_{name}"] / out[f"{tag}_ms_se_ard"]
    ctx.close()


batch_case("full", args.full, 2048, 6)
batch_case("mid", args.mid, 1024, 6)

# ---- sliding windows: push and forecast -------------------------------------------------------------------------------------------
W, N, d, T = args.windows, 512, 3, args.ticks
t = np.arange(11, 11 + N + T + 64 * (args.reps + 1), dtype=np.float64)
Xw = np.empty((W, len(t), d))
Xw[:, :, 0] = (t - t.mean()) / t.std()
Xw[:, :, 1:] = rng.normal(size=(W, len(t), d - 1))
yw = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (W, len(t)))
thw = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
dXw, dyw = torch.from_numpy(Xw).to(dev), torch.from_numpy(yw).to(dev)
Xq = np.empty((W, M, d))
Xq[:, :, 1:] = rng.normal(size=(W, M, d - 1))
ctxs = {}
for name, kid in KERNELS:
    c = engine.Context(max_n=8, max_m=8, max_d=d)
    c.window_init(W, N, d, kid, thw)
    ctxs[name] = c
pos = {name: 0 for name, _ in KERNELS}
pout = torch.empty((3, W, N), device=dev, dtype=torch.float64)


def push(name, n):
    a = pos[name]
    xs, ys = dXw[:, a:a + n].contiguous(), dyw[:, a:a + n].contiguous()
    ctxs[name].window_push_device(n, xs.data_ptr(), ys.data_ptr(), True, pout[0].data_ptr(), pout[1].data_ptr(), pout[2].data_ptr(), stream)
    pos[name] = a + n


for name, _ in KERNELS:
    push(name, N)
    push(name, T)
torch.cuda.synchronize()
ms = timed([(lambda n=name: push(n, 64)) for name, _ in KERNELS], args.reps)
for (name, kid), v in zip(KERNELS, ms):
    out[f"push_us_per_tick_{name}"] = v * 1e3 / 64
    assert ctxs[name].window_state(0)[1] == 0
end = pos["se_ard"]
assert all(p == end for p in pos.values())
Xq[:, :, 0] = ((t[end - 1] + 1 + np.arange(M)) - t.mean()) / t.std()
dXq = torch.from_numpy(Xq).to(dev)
fm = {name: torch.empty((2, W, M), device=dev, dtype=torch.float64) for name, _ in KERNELS}
ms = timed([(lambda n=name: ctxs[n].window_predict_device(M, dXq.data_ptr(), True, fm[n][0].data_ptr(), fm[n][1].data_ptr(), stream))
            for name, _ in KERNELS], args.reps)
for (name, kid), v in zip(KERNELS, ms):
    out[f"forecast_ms_{name}"] = v
    mv = fm[name].cpu().numpy()
    for w in sorted({0, W - 1}):
        f = oracle_fit(kid, thw, Xw[w, end - N:end], yw[w, end - N:end])
        omu, ovar = oracle_predict(kid, f, Xq[w])
        err = max(err, float(np.max(np.abs(mv[0, w] - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(mv[1, w] - ovar) / ovar)))
for what in ("push_us_per_tick", "forecast_ms"):
    for name in ("matern32", "matern52"):
        out[f"{what}_{name}_over_se_ard"] = out[f"{what}_{name}"] / out[f"{what}_se_ard"]

# ---- the node callback on one 134-sample window (host buffers, wall clock) -------------------------------------------------------
tt, ss = synth.reference_window()
node = engine.Context(max_n=256, max_m=1024, max_d=1, max_batch=1)
th1 = np.array([0.05, 25.0, 0.002])


def wall(fn, n):
    fn()
    t0 = time.perf_counter()
    for _ in range(n):
        r = fn()
    return (time.perf_counter() - t0) / n * 1e3, r


for name, kid in KERNELS:
    out[f"node_ms_{name}"], (m1, s1) = wall(lambda: node.slip_node_callback(tt, ss, th1, kernel_id=kid), 20)
    out[f"node_opt_ms_{name}"], (m2, s2, tho) = wall(lambda: node.slip_node_callback_opt(tt, ss, np.ones(3), kernel_id=kid), 5)
    ntr = int(0.9 * len(tt))
    _, _, nev = node.optimize(tt[:ntr], ss[:ntr], kid, np.ones(3))
    out[f"node_opt_evals_{name}"] = int(nev)
    Xtr, Xs1 = tt[:ntr, None], (tt.min() + len(tt) + np.arange(599.0))[:, None]
    for th_, m_, s_ in ((th1, m1, s1), (tho, m2, s2)):
        omu, ovar = oracle_predict(kid, oracle_fit(kid, th_, Xtr, ss[:ntr]), Xs1)
        err = max(err, float(np.max(np.abs(m_ - omu)) / np.max(np.abs(omu))), float(np.max(np.abs(s_ - 2 * np.sqrt(ovar)) / (2 * np.sqrt(ovar)))))
out["max_rel_err_vs_oracle"] = err
out["value"] = out["full_fits_per_s_matern52"]
print(json.dumps(out))
if not err < 1e-6:
    sys.exit("outputs disagree with the oracle: %g" % err)
