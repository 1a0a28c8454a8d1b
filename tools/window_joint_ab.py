#!/usr/bin/env python3
"""Bitwise A/B of the resident-window and joint-forecast kernels between two builds of the library.

    CGP_LIB=<library A> python tools/window_joint_ab.py run a.npz
    CGP_LIB=<library B> python tools/window_joint_ab.py run b.npz
    python tools/window_joint_ab.py compare a.npz b.npz [verdict.txt]

`run` sends a fixed list of calls through the library that CGP_LIB names (one process per library) and saves every output;
`compare` is tools/grad_path_ab.py's: one line per call, equal (np.array_equal, NaNs in equal places) or the largest difference
in ulps, non-zero exit when any call differs.  Shapes are the smallest that reach every branch of the shared pieces:
  batch joint  N = 9 (no full block of 16 columns, the masked tail only), 16 (one block, no tail), 130 (blocks and a tail);
               M = 1, 17 (two tiles of one super-tile), 65 (an off-diagonal super-tile pair), 130 (three super-tiles, ragged);
               every kernel id; CGP_SMALL=off so that every N takes the tiled schedules; a device-form call of three fits whose
               middle one is indefinite
  windows      capacity 33 and 64, d = 1 and 3, kernel ids 0, 2, 4: empty, after N / 2 ticks, after N + 5 ticks, and with one
               window failed by a theta of negative noise (a push feeds every window of the context, so no window can stay
               empty beside filled ones: the empty state is all three windows before the first push, which takes the same
               n <= 0 branches); capacity 528 and 1040 (k_window_refactor<8> and <16>); one sample
               call at M = 520 (k_window_joint_chol<8>)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_path_ab import compare, theta_of, window   # noqa: E402


def points_for(kid, X, M, rng):
    """RBF x Brownian: the ticks after the last sample; else points around the last inputs."""
    if kid == 2:
        return X[-1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    return X[rng.integers(max(0, len(X) - 50), len(X), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def flat(*parts):
    return np.concatenate([np.ravel(np.asarray(p, dtype=np.float64)) for p in parts])


def batch_calls(engine, out):
    B, S = 2, 3
    for N in (9, 16, 130):
        ctx = engine.Context(max_n=N, max_m=130, max_d=2, max_batch=3)
        assert ctx.joint_reserve(3, 130) == 0
        for kid in range(5):
            d = 1 if kid == 2 else 2
            Xw, Yw = zip(*[window(N, d, 40 * kid + N + b, kid) for b in range(B)])
            X, y = np.stack(Xw), np.stack([Y[0] for Y in Yw])
            theta = np.tile(theta_of(kid, d), (B, 1))
            for M in (1, 17, 65, 130):
                rng = np.random.default_rng(1000 * kid + N + M)
                Xs = np.stack([points_for(kid, X[b], M, rng) for b in range(B)])
                xi = rng.normal(size=(B, S, M))
                tag = f"kid{kid} N{N} M{M}"
                out[f"fit_predict_cov_batch {tag}"] = flat(*ctx.fit_predict_cov_batch(X, y, Xs, theta, kid))
                out[f"fit_sample_batch {tag}"] = flat(*ctx.fit_sample_batch(X, y, Xs, theta, kid, xi, include_noise=True))
                ctx.fit(X[0], y[0], kid, theta[0])
                out[f"predict_cov {tag}"] = flat(*ctx.predict_cov(Xs[0], include_noise=False))
                out[f"sample {tag}"] = flat(*ctx.sample(Xs[0], xi[0]))
        ctx.close()

    # device form: no jitter ladder, fit 1 stays indefinite -- NaN in its covariance and paths, its neighbours untouched
    import torch
    B, N, d, M, kid = 3, 130, 2, 65, 1
    Xw, Yw = zip(*[window(N, d, 70 + b, kid) for b in range(B)])
    X, y = np.stack(Xw), np.stack([Y[0] for Y in Yw])
    rng = np.random.default_rng(5)
    Xs = np.stack([points_for(kid, X[b], M, rng) for b in range(B)])
    th = np.zeros((B, 10))
    th[:, :4] = theta_of(kid, d)
    th[1, 3] = -2.0 * th[1, 0]
    dX, dy, dXs, dth, dxi = (torch.from_numpy(np.ascontiguousarray(a)).cuda()
                             for a in (X.transpose(0, 2, 1), y, Xs.transpose(0, 2, 1), th, rng.normal(size=(B, S, M))))
    dm, dc, dp = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((B, M), (B, M, M), (B, S, M)))
    dl = torch.zeros(B, dtype=torch.float64, device="cuda")
    di, ds = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B)
    assert ctx.joint_reserve(B, M) == 0
    args = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0)
    assert ctx.fit_predict_cov_batch_device(*args, True, dm.data_ptr(), dc.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
    assert ctx.fit_sample_batch_device(*args, True, S, dxi.data_ptr(), 1e-6, dp.data_ptr(), dl.data_ptr(), di.data_ptr(), ds.data_ptr()) == 0
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in (dm, dc, dp, dl, di, ds)]
    assert res[4][1] != 0 and res[4][0] == 0 and res[4][2] == 0 and np.all(np.isnan(res[1][1])) and np.all(np.isnan(res[2][1])), res[4]
    out["device form B3 N130 M65, fit 1 indefinite"] = flat(*res)
    ctx.close()


def window_round(ctx, out, tag, Xs, xi, theta):
    """Every call on the windows as they stand, a set_theta of every window in between."""
    out[f"window_predict_cov {tag}"] = flat(*ctx.window_predict_cov(Xs, check=False))
    out[f"window_sample {tag}"] = flat(*ctx.window_sample(Xs, xi, include_noise=True, check=False))
    out[f"window_nll_grad {tag}"] = flat(*ctx.window_nll_grad())
    out[f"window_loo {tag}"] = flat(*ctx.window_loo())
    out[f"window_set_theta {tag}"] = flat(*ctx.window_set_theta(theta, check=False))
    out[f"window_predict_cov after set_theta {tag}"] = flat(*ctx.window_predict_cov(Xs, include_noise=False, check=False))
    out[f"window_nll_grad after set_theta {tag}"] = flat(*ctx.window_nll_grad())
    out[f"window_loo after set_theta {tag}"] = flat(*ctx.window_loo())


def window_calls(engine, out):
    W, S = 3, 3
    for N in (33, 64):
        for kid, d in ((0, 1), (0, 3), (2, 1), (4, 1), (4, 3)):
            M = 70 if N == 33 else 20
            T = N + 5
            Xw, Yw = zip(*[window(T, d, 10 * kid + N + d + w, kid) for w in range(W)])
            X, y = np.stack(Xw), np.stack([Y[0] for Y in Yw])
            rng = np.random.default_rng(N + kid + d)
            Xs = np.stack([points_for(kid, X[w], M, rng) for w in range(W)])
            xi = rng.normal(size=(W, S, M))
            theta = np.tile(theta_of(kid, d), (W, 1))
            ctx = engine.Context(max_n=8, max_m=8, max_d=d)
            ctx.window_init(W, N, d, kid, theta)
            assert ctx.window_joint_reserve(M) == 0
            tag = f"kid{kid} N{N} d{d}"
            window_round(ctx, out, tag + " empty", Xs, xi, theta * 1.1)
            ctx.window_push(X[:, :N // 2], y[:, :N // 2])
            window_round(ctx, out, tag + " filling", Xs, xi, theta * 1.2)
            ctx.window_push(X[:, N // 2:], y[:, N // 2:])
            window_round(ctx, out, tag + " origin moved", Xs, xi, theta * 1.3)
            bad = theta.copy()
            bad[1, -1] = -2.0 * bad[1, 0]   # window 1's Ky is negative definite: repaired, reported, NaN from then on
            ctx.window_set_theta(bad, check=False)
            window_round(ctx, out, tag + " window 1 failed", Xs, xi, bad)
            assert ctx.window_state(1)[1] != 0 and ctx.window_state(0)[1] == 0
            ctx.close()

    # the 8 and 16 tiles-per-wave factorisations of k_window_refactor, SE-ARD and Matern 5/2
    d, M = 2, 20
    for N, T in ((528, 600), (1040, 1100)):
        for kid in (1, 4):
            X, Y = window(T, d, N + kid, kid)
            rng = np.random.default_rng(N)
            Xs = points_for(kid, X, M, rng)[None]
            theta = theta_of(kid, d)[None]
            ctx = engine.Context(max_n=8, max_m=8, max_d=d)
            ctx.window_init(1, N, d, kid, theta)
            assert ctx.window_joint_reserve(M) == 0
            ctx.window_push(X[None], Y[:1])
            window_round(ctx, out, f"kid{kid} N{N} d{d}", Xs, rng.normal(size=(1, S, M)), theta * 1.2)
            ctx.close()

    # the 8 tiles-per-wave factorisation of k_window_joint_chol
    N, d, M, kid = 33, 2, 520, 0
    X, Y = window(N + 5, d, 77, kid)
    rng = np.random.default_rng(77)
    Xs = points_for(kid, X, M, rng)[None]
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta_of(kid, d)[None])
    assert ctx.window_joint_reserve(M) == 0
    ctx.window_push(X[None], Y[:1])
    out[f"window_sample kid{kid} N{N} d{d} M{M} S{S}"] = flat(*ctx.window_sample(Xs, rng.normal(size=(1, S, M)), include_noise=True, check=False))
    ctx.close()


def run(out_path):
    os.environ["CGP_SMALL"] = "off"
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, which has to be the process's first)
    import corenav_gp_amd.engine as engine
    engine.load()
    out = {}
    batch_calls(engine, out)
    window_calls(engine, out)
    np.savez(out_path, **out)
    print(f"{len(out)} calls saved to {out_path} (library {engine.LIB_PATH})")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
