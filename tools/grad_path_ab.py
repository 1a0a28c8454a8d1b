#!/usr/bin/env python3
"""Bitwise A/B of the gradient path between two builds of the library.

    CGP_LIB=<library A> python tools/grad_path_ab.py run a.npz
    CGP_LIB=<library B> python tools/grad_path_ab.py run b.npz
    python tools/grad_path_ab.py compare a.npz b.npz [verdict.txt]

`run` sends a fixed list of calls through the library that CGP_LIB names (one process per library) and saves every output;
`compare` prints one line per call: equal (np.array_equal, NaNs in equal places), or the largest difference in ulps, and exits
non-zero when any call differs.  Shapes are the smallest that reach every branch of the 128 x 128 tile contraction: N = 129 (an
off-diagonal pair with one live row), 257 (a pair away from the diagonal), 300 (a ragged last tile).  The process runs with
CGP_SMALL=off so that every N takes the tiled schedules and the host optimiser."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (129, 257, 300)


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])


def window(N, d, seed, kid=1, P=1):
    """Inputs (N, d) -- ticks for the Brownian kernel -- and P smooth noisy target columns (P, N)."""
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + N, dtype=np.float64)
    X = t[:, None] if kid == 2 else np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)])
    ph = rng.random((P, 1)) * 6.0
    Y = 0.1 * np.sin(0.05 * t[None] + ph) + 0.03 * np.cos(0.31 * t[None] * (1.0 + ph)) + 0.01 * rng.normal(size=(P, N))
    return X, Y


def ladder_batch(N, P):
    """Three fits of d = 1, SE: fit 1 has duplicated inputs and sigma_n^2 = 1e-10 under a large amplitude (needs the jitter
    ladder), fit 2 a negative noise (stays indefinite)."""
    rng = np.random.default_rng(21)
    X = np.stack([np.sort(rng.normal(size=(N, 1)), 0) for _ in range(3)])
    X[1, :, 0] = np.repeat(np.arange((N + 1) // 2, dtype=float), 2)[:N]
    Y = np.stack([np.sin((1.0 + 0.1 * p) * X[:, :, 0]) + 0.1 * p for p in range(P)], axis=1)
    th = np.array([[1.0, 1.0, 0.05], [1e9, 3.0, 1e-10], [1.0, 1.0, 0.05]])
    return X, Y, th


def run(out_path):
    os.environ["CGP_SMALL"] = "off"
    sys.path.insert(0, ROOT)
    import corenav_gp_amd.engine as engine
    engine.load()
    out = {}

    # cgp_nll_grad: every kernel id, d = 1, 3, 8, fp64; SE-ARD in an fp32 context
    for N in NS:
        ctx = engine.Context(max_n=N, max_m=N, max_d=8)
        for kid in range(5):
            for d in ((1,) if kid == 2 else (1, 3, 8)):
                X, Y = window(N, d, 100 * kid + d, kid)
                nll, g = ctx.nll_grad(X, Y[0], kid, theta_of(kid, d))
                out[f"nll_grad f64 kid{kid} d{d} N{N}"] = np.concatenate([[nll], g])
        ctx.close()
        ctx = engine.Context(max_n=N, max_m=N, max_d=3, dtype=engine.F32)
        X, Y = window(N, 3, 7)
        nll, g = ctx.nll_grad(X, Y[0], 1, theta_of(1, 3))
        out[f"nll_grad f32 kid1 d3 N{N}"] = np.concatenate([[nll], g])
        ctx.close()

    # cgp_multi_nll_grad_batch: P = 1, 17, 129; one fit alone, and three of which one needs the ladder and one stays indefinite
    for P in (1, 17, 129):
        for kid, d, N in ((1, 3, 129), (3, 3, 300), (2, 1, 257)):
            ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=1)
            assert ctx.multi_reserve(1, P) == 0 and ctx.multi_grad_reserve(1, P) == 0
            X, Y = window(N, d, 300 + P + kid, kid, P)
            rc, nll, g, lml, info = ctx.multi_nll_grad_batch(X[None], Y[None], theta_of(kid, d)[None], kid)
            out[f"multi_nll_grad B1 kid{kid} N{N} P{P}"] = np.concatenate([[rc], nll, g.ravel(), lml.ravel(), info])
            ctx.close()
        N = 257
        X, Y, th = ladder_batch(N, P)
        th[2, -1] = -2.0 * th[2, 0]
        ctx = engine.Context(max_n=N, max_m=N, max_d=1, max_batch=3)
        assert ctx.multi_reserve(3, P) == 0 and ctx.multi_grad_reserve(3, P) == 0
        rc, nll, g, lml, info = ctx.multi_nll_grad_batch(X, Y, th, 0)
        assert info[0] == 0 and info[1] == 0 and info[2] != 0 and np.isfinite(nll[1]), (info, nll)
        out[f"multi_nll_grad B3 ladder + indefinite N{N} P{P}"] = np.concatenate([[rc], nll, g.ravel(), lml.ravel(), info])
        ctx.close()

    # the three batched optimisers, max_evals = 12 (only cgp_window_optimize takes a select mask)
    N = 129
    Xw, Yw = zip(*[window(N, 2, 500 + b) for b in range(3)])
    ctx = engine.Context(max_n=N, max_m=N, max_d=2, max_batch=3)
    th, lml, nev = ctx.optimize_batch(np.stack(Xw), np.stack([y[0] for y in Yw]), 1, np.array([0.05, 1.0, 1.0, 0.01]), max_evals=12)
    out["optimize_batch kid1 B3 N129"] = np.concatenate([th.ravel(), lml, nev])
    ctx.close()
    X, Y, th0 = ladder_batch(N, 2)   # window 1 starts where the whole-batch / per-fit ladder has to climb
    ctx = engine.Context(max_n=N, max_m=N, max_d=1, max_batch=3)
    th, lml, nev = ctx.optimize_batch(X, Y[:, 0], 0, th0, max_evals=12)
    out["optimize_batch kid0 B3 N129 ladder"] = np.concatenate([th.ravel(), lml, nev])
    assert ctx.multi_reserve(3, 2) == 0 and ctx.multi_grad_reserve(3, 2) == 0
    th, lml, nev = ctx.optimize_multi_batch(X, Y, 0, th0, max_evals=12)
    out["optimize_multi_batch kid0 B3 N129 P2 ladder"] = np.concatenate([th.ravel(), lml, nev])
    ctx.close()
    W, Nw, d, T = 3, 192, 3, 260
    Xw, Yw = zip(*[window(T, d, 600 + w) for w in range(W)])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, Nw, d, 1, np.tile(np.array([0.05, 1.0, 1.0, 1.0, 0.01]), (W, 1)))
    ctx.window_push(np.stack(Xw), np.stack([y[0] for y in Yw]))
    th, lml, nev = ctx.window_optimize(max_evals=12, select=np.array([1, 0, 1], dtype=bool))
    nll, g = ctx.window_nll_grad()   # the factors the windows are left with
    out["window_optimize kid1 W3 N192 select 1 0 1"] = np.concatenate([th.ravel(), lml, nev, nll, g.ravel()])
    ctx.close()

    # cgp_loo_batch and cgp_fit_predict_batch with one fit that needs jitter
    N = 257
    X, Y, th = ladder_batch(N, 1)
    ctx = engine.Context(max_n=N, max_m=N, max_d=1, max_batch=3)
    res = ctx.loo_batch(X, Y[:, 0], th, 0)
    assert res[0] == 0 and not res[-1].any()
    out["loo_batch B3 N257 ladder"] = np.concatenate([np.ravel(r) for r in res])
    Xs = X[:, ::16] + 0.01
    res = ctx.fit_predict_batch(X, Y[:, 0], Xs, th, 0)
    assert res[0] == 0 and not res[-1].any()
    out["fit_predict_batch B3 N257 M17 ladder"] = np.concatenate([np.ravel(r) for r in res])
    ctx.close()

    np.savez(out_path, **{k: np.asarray(v, dtype=np.float64) for k, v in out.items()})
    print(f"{len(out)} calls saved to {out_path} (library {engine.LIB_PATH})")


def ulps(a, b):
    """Largest distance in units in the last place between two fp64 arrays (NaN against a number: inf)."""
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return np.inf
    def key(v):
        i = v.view(np.int64)
        return np.where(i < 0, np.int64(-2**63) - i, i).astype(np.float64)   # ordered like the values
    ok = ~na
    return float(np.max(np.abs(key(a[ok]) - key(b[ok])))) if ok.any() else 0.0


def compare(pa, pb, verdict=None):
    a, b = np.load(pa), np.load(pb)
    lines, bad = [], 0
    if sorted(a.files) != sorted(b.files):
        lines.append("the two runs hold different calls")
        bad += 1
    for k in a.files:
        if k not in b.files:
            continue
        if a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True):
            lines.append(f"{k}: equal ({a[k].size} values)")
        else:
            bad += 1
            lines.append(f"{k}: DIFFERENT, " + (f"largest difference {ulps(a[k], b[k]):.0f} ulps" if a[k].shape == b[k].shape else "shapes differ"))
    lines.append(f"{len(a.files)} calls, {bad} different")
    text = "\n".join(lines)
    print(text)
    if verdict:
        with open(verdict, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
