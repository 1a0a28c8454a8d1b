#!/usr/bin/env python3
"""Benchmark of the explicit-basis (trend) calls beside the route a caller has without them, in one process on the same samples
(same-process A/B: one box, one clock state).  fp64, SE-ARD, device-resident, the host clock around each route and a synchronisation, after warm-up.

The route of today: the multi-target call over [Y | H] and the columns that expose the inner products the epilogue needs -- the
call returns |Z_j|^2 only, inside logml, so G^T G and G^T Z are recovered by polarisation from the extra columns H_r + H_s (r < s),
Y_p + H_r and one zero column (which gives sum log L_ii) --, a copy back of mean / var / logml, and the q x q epilogue in numpy on
the host.  The trend call: cgp_fit_predict_trend_batch_device and the same copy back of its outputs.

  batch fits: N = 2048, d = 6, M = 599, q = 2 at (1 fit, P = 4) and (64 fits, P = 4)
  windows:    N = 512, d = 2, M = 599, q = 2, P - q = 4 targets at 1 and 64 windows (cgp_window_predict_trend_device against
              cgp_window_predict_multi_device over the same extended columns)
Prints ONE JSON line and writes it to --out (profiles/trend_bench.json):
  shapes[]: what, fits, P, q, trend_ms, multi_ms (the multi-target call over the P + q columns alone: what the trend call is built on),
            today_ms (extended multi call + copy back + numpy epilogue), trend_over_multi, today_over_trend, routes_max_rel_diff
            (host clock around call + synchronise; trend_ms and today_ms include the copy back of the outputs, multi_ms does not)
  max_err_over_bar: the timed trend outputs of the first shape against tests/trend_oracle.py on fit 0, in units of the 1e-6 bar; the
            tool fails beyond 1.  No ratio is required: the expectation is that the multi-target call's time dominates."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--wn", type=int, default=512)
ap.add_argument("--m", type=int, default=599)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fits", type=str, default="1,64")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "trend_bench.json"))
args = ap.parse_args()
import torch
import corenav_gp_amd.engine as engine
import trend_oracle as to   # checker only, after the timed regions
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(20271)
M, P, q, kid = args.m, 4, 2, engine.KERNEL_SE_ARD
FITS = [int(b) for b in args.fits.split(",")]
BMAX = max(FITS)
LOG_2PI = float(np.log(2.0 * np.pi))
f64 = dict(device=dev, dtype=torch.float64)
PAIRS = [(r, s) for r in range(q) for s in range(r + 1, q)]
PE = P + q + len(PAIRS) + P * q + 1   # [Y | H | H_r + H_s | Y_p + H_r | 0]


def timed(call, n):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def extended(Y, H):
    """(.., P, n), (.., q, n) -> (.., PE, n)"""
    cols = [Y, H] + [H[..., r:r + 1, :] + H[..., s:s + 1, :] for r, s in PAIRS]
    cols += [Y[..., p:p + 1, :] + H[..., r:r + 1, :] for p in range(P) for r in range(q)] + [np.zeros_like(H[..., :1, :])]
    return np.concatenate(cols, axis=-2)


def epilogue(mean, var, logml, Hs, n):
    """The host epilogue of today's route, per fit: the multi-target outputs of the extended columns -> mean, var, beta, logml."""
    B = mean.shape[0]
    om, ov, ob, ol = np.empty((B, P, M)), np.empty((B, M)), np.empty((B, P, q)), np.empty((B, P))
    for b in range(B):
        base = logml[b, -1]                       # -sum log L_ii - n/2 log 2 pi
        zz = -2.0 * (logml[b] - base)             # |Z_j|^2 of every column
        A, Bm = np.empty((q, q)), np.empty((q, P))
        for r in range(q):
            A[r, r] = zz[P + r]
        for i, (r, s) in enumerate(PAIRS):
            A[r, s] = A[s, r] = 0.5 * (zz[P + q + i] - zz[P + r] - zz[P + s])
        for p in range(P):
            for r in range(q):
                Bm[r, p] = 0.5 * (zz[P + q + len(PAIRS) + p * q + r] - zz[p] - zz[P + r])
        LA = np.linalg.cholesky(A)
        Wm = np.linalg.solve(LA, Bm)
        beta = np.linalg.solve(LA.T, Wm)
        R = Hs[b] - mean[b, P:P + q]
        U = np.linalg.solve(LA, R)
        om[b] = mean[b, :P] + beta.T @ R
        ov[b] = var[b] + np.sum(U * U, 0)
        ob[b] = beta.T
        ol[b] = logml[b, :P] + 0.5 * np.sum(Wm * Wm, 0) - np.sum(np.log(np.diag(LA))) + 0.5 * q * LOG_2PI
    return om, ov, ob, ol


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


out = {"metric": "trend-vs-multi-plus-host-epilogue", "M": M, "P": P, "q": q, "kernel": "se_ard", "extended_columns": PE, "shapes": []}
first = None

# ---- batch fits ------------------------------------------------------------------------------------------------------------------
N, d = args.n, 6
X = rng.uniform(-2.0, 2.0, (BMAX, N, d))
Xs = rng.uniform(-2.0, 2.5, (BMAX, M, d))
Wt = rng.normal(size=(BMAX, d, P))
Y = np.sin(X @ Wt).transpose(0, 2, 1) + 0.4 + 0.3 * X[:, None, :, 0] + 0.05 * rng.normal(size=(BMAX, P, N))
H = np.stack([np.ones((BMAX, N)), X[:, :, 0]], axis=1)
Hs = np.stack([np.ones((BMAX, M)), Xs[:, :, 0]], axis=1)
th = np.column_stack([rng.uniform(0.5, 1.5, BMAX)] + [rng.uniform(1.0, 3.0, BMAX) for _ in range(d)] + [np.full(BMAX, 0.01)])
thp = np.zeros((BMAX, engine.MAX_THETA))
thp[:, :d + 2] = th
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
dX, dXs, dY, dH, dHs, dth = up(X.transpose(0, 2, 1)), up(Xs.transpose(0, 2, 1)), up(Y), up(H), up(Hs), up(thp)
dYH, dYE = up(np.concatenate([Y, H], axis=1)), up(extended(Y, H))
ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=BMAX)
ctx.multi_reserve(BMAX, PE + 16)
ctx.trend_reserve(BMAX, P, M)
for B in FITS:
    tm, tv, tb, tl = torch.empty((B, P, M), **f64), torch.empty((B, M), **f64), torch.empty((B, P, q), **f64), torch.empty((B, P), **f64)
    ti, tt = torch.zeros(B, device=dev, dtype=torch.int32), torch.zeros(B, device=dev, dtype=torch.int32)
    em, ev, el = torch.empty((B, PE, M), **f64), torch.empty((B, M), **f64), torch.empty((B, PE), **f64)
    res = {}

    def run_trend():
        ctx.fit_predict_trend_batch_device(B, N, d, M, P, q, kid, dX.data_ptr(), dY.data_ptr(), dH.data_ptr(), dXs.data_ptr(), dHs.data_ptr(),
                                           dth.data_ptr(), 0, True, tm.data_ptr(), tv.data_ptr(), tb.data_ptr(), tl.data_ptr(), ti.data_ptr(),
                                           tt.data_ptr(), stream)
        res["trend"] = [t.cpu().numpy() for t in (tm, tv, tb, tl)]

    def run_multi():   # the call the trend call is built on, over [Y | H] alone, outputs left on the device
        ctx.fit_predict_multi_batch_device(B, N, d, M, P + q, kid, dX.data_ptr(), dYH.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                           em.data_ptr(), ev.data_ptr(), el.data_ptr(), ti.data_ptr(), stream)

    def run_today():
        ctx.fit_predict_multi_batch_device(B, N, d, M, PE, kid, dX.data_ptr(), dYE.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                           em.data_ptr(), ev.data_ptr(), el.data_ptr(), ti.data_ptr(), stream)
        res["today"] = epilogue(em.cpu().numpy(), ev.cpu().numpy(), el.cpu().numpy(), Hs[:B], N)

    rec = {"what": "batch", "N": N, "d": d, "fits": B, "trend_ms": timed(run_trend, args.reps), "multi_ms": timed(run_multi, args.reps),
           "today_ms": timed(run_today, args.reps)}
    assert not ti.cpu().numpy().any() and not tt.cpu().numpy().any()
    rec["trend_over_multi"] = rec["trend_ms"] / rec["multi_ms"]
    rec["today_over_trend"] = rec["today_ms"] / rec["trend_ms"]
    rec["routes_max_rel_diff"] = max(rel(a, b) for a, b in zip(res["today"], res["trend"]))
    out["shapes"].append(rec)
    if first is None:
        first = res["trend"]
o = to.fit_predict_trend(kid, th[0], X[0], Y[0], H[0], Xs[0], Hs[0], True)
assert to.conditions_hold(o), (o.cond, o.margin, o.jitter)
out["max_err_over_bar"] = float(max(to.errors(first[0][0], first[1][0], first[2][0], first[3][0], o))) / 1e-6
ctx.close()

# ---- resident windows ------------------------------------------------------------------------------------------------------------
N, d = args.wn, 2
for Wn in FITS:
    t = np.arange(11, 11 + N, dtype=np.float64)
    Xw = np.empty((Wn, N, d))
    Xw[:, :, 0] = (t - t.mean()) / t.std()
    Xw[:, :, 1] = rng.normal(size=(Wn, N))
    Yw = np.sin(2.0 * Xw[:, None, :, 0] + np.arange(P)[None, :, None]) * 0.1 + 0.1 + 0.05 * Xw[:, None, :, 0] + 0.01 * rng.normal(size=(Wn, P, N))
    Hw = np.stack([np.ones((Wn, N)), Xw[:, :, 0]], axis=1)
    Xq = np.stack([np.linspace(1.7, 3.0, M)[None].repeat(Wn, 0), rng.normal(size=(Wn, M))], axis=2)
    Hq = np.stack([np.ones((Wn, M)), Xq[:, :, 0]], axis=1)
    theta = np.array([0.02, 0.8, 1.6, 1e-3])
    dxq, dhq = up(Xq), up(Hq)
    res = {}
    ct = engine.Context(max_n=8, max_m=8, max_d=d)
    ct.window_init(Wn, N, d, kid, theta)
    ct.window_multi_reserve(P + q)
    ct.window_trend_reserve(q, M)
    ct.window_push_multi(Xw, np.concatenate([Yw, Hw], axis=1).transpose(0, 2, 1))
    ce = engine.Context(max_n=8, max_m=8, max_d=d)
    ce.window_init(Wn, N, d, kid, theta)
    ce.window_multi_reserve(PE)
    ce.window_push_multi(Xw, extended(Yw, Hw).transpose(0, 2, 1))
    tm, tv, tb, tl = torch.empty((Wn, P, M), **f64), torch.empty((Wn, M), **f64), torch.empty((Wn, P, q), **f64), torch.empty((Wn, P), **f64)
    tt = torch.zeros(Wn, device=dev, dtype=torch.int32)
    mm, ml = torch.empty((Wn, P + q, M), **f64), torch.empty((Wn, P + q), **f64)
    em, ev, el = torch.empty((Wn, PE, M), **f64), torch.empty((Wn, M), **f64), torch.empty((Wn, PE), **f64)

    def win_trend():
        ct.window_predict_trend_device(M, P + q, q, dxq.data_ptr(), dhq.data_ptr(), True, tm.data_ptr(), tv.data_ptr(), tb.data_ptr(),
                                       tl.data_ptr(), tt.data_ptr(), stream)
        res["trend"] = [x.cpu().numpy() for x in (tm, tv, tb, tl)]

    def win_multi():
        ct.window_predict_multi_device(M, P + q, dxq.data_ptr(), True, mm.data_ptr(), ev.data_ptr(), ml.data_ptr(), stream)

    def win_today():
        ce.window_predict_multi_device(M, PE, dxq.data_ptr(), True, em.data_ptr(), ev.data_ptr(), el.data_ptr(), stream)
        res["today"] = epilogue(em.cpu().numpy(), ev.cpu().numpy(), el.cpu().numpy(), Hq, N)

    rec = {"what": "windows", "N": N, "d": d, "fits": Wn, "trend_ms": timed(win_trend, args.reps), "multi_ms": timed(win_multi, args.reps),
           "today_ms": timed(win_today, args.reps)}
    assert not tt.cpu().numpy().any()
    rec["trend_over_multi"] = rec["trend_ms"] / rec["multi_ms"]
    rec["today_over_trend"] = rec["today_ms"] / rec["trend_ms"]
    rec["routes_max_rel_diff"] = max(rel(a, b) for a, b in zip(res["today"], res["trend"]))
    out["shapes"].append(rec)
    ct.close()
    ce.close()

print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
sys.exit(0 if out["max_err_over_bar"] <= 1.0 else 1)
