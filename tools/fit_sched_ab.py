#!/usr/bin/env python3
"""Bitwise A/B of the fit schedules between two builds of the library, and their launch listings.

    CGP_LIB=<library A> python tools/fit_sched_ab.py run a.npz            # the shipped library's call list
    CGP_LIB=<library B> python tools/fit_sched_ab.py run b.npz
    python tools/fit_sched_ab.py compare a.npz b.npz [verdict.txt]        # tools/grad_path_ab.py's compare
    CGP_LIB=<ab library> CGP_SCHED=overlap python tools/fit_sched_ab.py run-switch a.npz    # one measurement switch per process
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/fit_sched_ab.py run-once
    python tools/fit_sched_ab.py listing <dir>/.../t_kernel_trace.csv > a.txt           # then diff a.txt b.txt

`run` sends a fixed list of small calls that reach every branch of sched_plan (corenav_gp_amd/csrc/cgp_sched_plan.hpp) through
the library that CGP_LIB names and saves every output: N = 100 ... 400 (1 ... 4 block steps), 897 (8 block steps), SE-ARD and
the Matern 3/2 kernel in fp64, SE-ARD in fp32, with CGP_SMALL=off so that every N takes the tiled schedules.  Results are bitwise
the same for either stream-group count, so the tuner's timing does not matter.  `run-switch` makes the two calls one switch of
the measurement library is checked on (CGP_SCHED=onelaunch: the two shapes of its own test).  `run-once` makes one call per
schedule with the stream groups fixed by cgp_set_streams (the tuner stays out of it); `listing` condenses the kernel trace of
such a run into kernel name, grid, workgroup size and LDS bytes per stream, in launch order, streams numbered by first use."""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_path_ab import compare, ladder_batch, theta_of, window   # noqa: E402


def batch_of(B, N, d, M, kid, seed):
    Xw, Yw = zip(*[window(N, d, seed + b, kid) for b in range(B)])
    X, y = np.stack(Xw), np.stack([Y[0] for Y in Yw])
    Xs = X[:, np.linspace(0, N - 1, M).astype(int)] + 0.013
    return X, y, Xs, np.tile(theta_of(kid, d), (B, 1))


def engine_of():
    os.environ["CGP_SMALL"] = "off"
    sys.path.insert(0, ROOT)
    import corenav_gp_amd.engine as engine
    engine.load()
    return engine


def call(engine, out, key, dtype, B, N, M=5, kid=1, d=2, streams=None, refine=None, prof=False):
    """One cgp_fit_predict_batch call in a context made for it; with prof, its cgp_profile_read launch counts too."""
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B, dtype=dtype)
    if streams is not None:
        ctx.set_streams(streams)
    if refine is not None:
        ctx.set_refine(refine)
    if prof:
        ctx.profile_enable(True)
    X, y, Xs, th = batch_of(B, N, d, M, kid, 1000 + N + B)
    rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th, kid)
    res = [[rc], mean.ravel(), var.ravel(), logml, info]
    if prof:
        res.append([v["launches"] for v in ctx.profile_read().values()])
    out[key] = np.concatenate(res)
    ctx.close()


def single(engine, out, key, dtype, N, M, kid=1, d=2, refine=None):
    """cgp_fit + cgp_predict + cgp_get_alpha: predict after fit."""
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, dtype=dtype)
    if refine is not None:
        ctx.set_refine(refine)
    X, y, Xs, th = batch_of(1, N, d, M, kid, 2000 + N + M)
    rc, logml = ctx.fit(X[0], y[0], kid, th[0])
    mean, var = ctx.predict(Xs[0])
    out[key] = np.concatenate([[rc, logml], mean, var, ctx.alpha()])
    ctx.close()


def run(out_path):
    engine = engine_of()
    F64, F32 = engine.F64, engine.F32
    out = {}
    for kid in (1, 3):   # SE-ARD, Matern 3/2
        t = f"f64 kid{kid}"
        for N, B in ((100, 1), (100, 48), (130, 3), (300, 2), (300, 28)):
            call(engine, out, f"{t} latency N{N} x{B}", F64, B, N, kid=kid)
        for N, B in ((300, 29), (300, 48), (400, 30)):
            call(engine, out, f"{t} mid-size N{N} x{B}", F64, B, N, kid=kid)
        for M in (5, 130):
            call(engine, out, f"{t} mid-size, extra rows split N897 x60 M{M}", F64, 60, 897, M=M, kid=kid)
            call(engine, out, f"{t} mid-size, profiled N897 x60 M{M}", F64, 60, 897, M=M, kid=kid, prof=True)
        call(engine, out, f"{t} full batch, fused diagonal N300 x49", F64, 49, 300, kid=kid)
        for n in (1, 2, 4):
            call(engine, out, f"{t} full batch, fused diagonal N300 x53 streams {n}", F64, 53, 300, kid=kid, streams=n)
        call(engine, out, f"{t} full batch, split diagonal N257 x512", F64, 512, 257, kid=kid)
        for M in (5, 130):
            single(engine, out, f"{t} fit + predict + alpha N300 M{M}", F64, 300, M, kid=kid)
    call(engine, out, "f32 latency N300 x24", F32, 24, 300)
    for B in (25, 56, 64, 96):
        for n in (1, 2):
            call(engine, out, f"f32 mid-size N300 x{B} streams {n}", F32, B, 300, streams=n)
    call(engine, out, "f32 full batch N300 x97", F32, 97, 300)
    for d in (1, 4):
        for r in (0, 1, 2):
            call(engine, out, f"f32 refine {r} d{d} N300 x4", F32, 4, 300, d=d, refine=r)
    call(engine, out, "f32 refine default N300 x64", F32, 64, 300)
    call(engine, out, "f32 refine default d4 N300 x64", F32, 64, 300, d=4)
    single(engine, out, "f32 fit + predict + alpha, refined N300 M5", F32, 300, 5)
    single(engine, out, "f32 fit + predict + alpha, unrefined N300 M5", F32, 300, 5, refine=0)
    # one fit needs the first rung of the jitter ladder, one stays indefinite
    X, Y, th = ladder_batch(257, 1)
    th[2, -1] = -2.0 * th[2, 0]
    ctx = engine.Context(max_n=257, max_m=17, max_d=1, max_batch=3)
    res = ctx.fit_predict_batch(X, Y[:, 0], X[:, ::16] + 0.01, th, 0)
    assert res[-1][0] == 0 and res[-1][1] == 0 and res[-1][2] != 0, res[-1]
    out["f64 kid0 N257 x3 ladder + indefinite"] = np.concatenate([np.ravel(r) for r in res])
    ctx.close()
    save(out, out_path, engine)


def run_switch(out_path):
    engine = engine_of()
    out = {}
    if os.environ.get("CGP_SCHED") == "onelaunch":
        call(engine, out, "f32 N640 x40", engine.F32, 40, 640)
        call(engine, out, "f64 N768 x24", engine.F64, 24, 768)
    else:
        call(engine, out, "f64 N300 x2", engine.F64, 2, 300)
        call(engine, out, "f32 N300 x2", engine.F32, 2, 300)
    save(out, out_path, engine)


def run_once():
    engine = engine_of()
    F64, F32 = engine.F64, engine.F32
    out = {}
    call(engine, out, "latency", F64, 2, 300, streams=1)
    call(engine, out, "mid-size", F64, 29, 300, streams=1)
    call(engine, out, "mid-size, extra rows split", F64, 60, 897, M=130, streams=1)
    call(engine, out, "mid-size, Matern", F64, 29, 300, kid=3, streams=1)
    call(engine, out, "full batch, two groups", F64, 53, 300, streams=2)
    call(engine, out, "full batch, split diagonal", F64, 512, 257, streams=1)
    single(engine, out, "predict after fit", F64, 300, 130)
    call(engine, out, "f32 latency", F32, 24, 300, streams=1)
    call(engine, out, "f32 mid-size, two groups", F32, 64, 300, streams=2)
    call(engine, out, "f32 mid-size, one group, gated refinement", F32, 64, 300, d=4, streams=1)
    call(engine, out, "f32 full batch", F32, 97, 300, streams=1)
    single(engine, out, "f32 predict after fit", F32, 300, 5)
    print(f"{len(out)} calls made (library {engine.LIB_PATH})")


def save(out, out_path, engine):
    np.savez(out_path, **{k: np.asarray(v, dtype=np.float64) for k, v in out.items()})
    print(f"{len(out)} calls saved to {out_path} (library {engine.LIB_PATH})")


def listing(path):
    def col(r, *names):
        return next((r[n] for n in names if n in r), "?")
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(col(r, "Dispatch_Id", "Start_Timestamp")))
    streams = {}
    for r in rows:
        streams.setdefault(col(r, "Stream_Id", "Queue_Id"), []).append(
            f"{col(r, 'Kernel_Name')}  grid {'x'.join(col(r, 'Grid_Size_' + a) for a in 'XYZ')}  "
            f"workgroup {'x'.join(col(r, 'Workgroup_Size_' + a) for a in 'XYZ')}  LDS {col(r, 'LDS_Block_Size', 'Group_Segment_Size')}")
    for i, launches in enumerate(streams.values()):
        print(f"stream {i}: {len(launches)} launches")
        print("\n".join("  " + l for l in launches))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "run" and len(sys.argv) >= 3:
        run(sys.argv[2])
    elif mode == "run-switch" and len(sys.argv) >= 3:
        run_switch(sys.argv[2])
    elif mode == "run-once":
        run_once()
    elif mode == "listing" and len(sys.argv) >= 3:
        listing(sys.argv[2])
    elif mode == "compare" and len(sys.argv) >= 4:
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
