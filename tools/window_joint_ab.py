#!/usr/bin/env python3
"""Bitwise A/B of the resident-window and joint-forecast kernels between two builds of the library.

    CGP_LIB=<library A> python tools/window_joint_ab.py run a.npz
    CGP_LIB=<library B> python tools/window_joint_ab.py run b.npz
    python tools/window_joint_ab.py compare a.npz b.npz [verdict.txt]
    CGP_LIB=<library> python tools/window_joint_ab.py run-windows-once a.npz     (the window calls at one shape: for a kernel trace)

`run` sends a fixed list of calls through the library that CGP_LIB names (one process per library) and saves every output;
`compare` is tools/grad_path_ab.py's: one line per call, equal (np.array_equal, NaNs in equal places) or the largest difference
in ulps, non-zero exit when any call differs.  Shapes are the smallest that reach every branch of the shared pieces:
  batch joint  N = 9 (no full block of 16 columns, the masked tail only), 16 (one block, no tail), 130 (blocks and a tail);
               M = 1, 17 (two tiles of one super-tile), 65 (an off-diagonal super-tile pair), 130 (three super-tiles, ragged);
               every kernel id; CGP_SMALL=off so that every N takes the tiled schedules; a device-form call of three fits whose
               middle one is indefinite
  hooked calls the multi-target calls (N = 130, M = 17, P = 1 / 17 / 129, the solve's tile height free, 64 and 128) and the
               predictive-gradient calls (N = 130, M = 1 / 65 / 130), host and device form, and cgp_predict_gradients: three
               fits, one retried on the ladder's first rung (the host form runs its post-fit hook again) and one indefinite
  windows      capacity 33 and 64, d = 1 and 3, kernel ids 0, 2, 4: empty, after N / 2 ticks, after N + 5 ticks, and with one
               window failed by a theta of negative noise (a push feeds every window of the context, so no window can stay
               empty beside filled ones: the empty state is all three windows before the first push, which takes the same
               n <= 0 branches); capacity 528 and 1040 (k_window_refactor<8> and <16>); one sample
               call at M = 520 (k_window_joint_chol<8>)
  window host  every entry point of the windows' host layer, host and device form, over the same four states at capacity 33 and
               64: the pushes (T = 1, N / 2, N + 5), forecasts and predictive gradients at M = 1 / 20 / 70, the leave-one-out
               objective with and without logml, the three optimisers at 12 evaluations, the multi-target family at P = 1 / 17;
               one push and one forecast staged by copy (above 16 KiB) at capacity 528 (window_host_calls)"""
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


def hooked_calls(engine, out):
    """The multi-target and predictive-gradient calls (the batch entry points with a post-fit hook besides the joint ones), host
    and device form, on three fits of N = 130: fit 0 factors, fit 1 needs exactly the ladder's first rung (the host form retries
    it once and runs the hook again for it alone), fit 2 stays indefinite on every rung.  tests/failure_oracle.py builds them."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import failure_oracle as fo
    B, N, d, kid = 3, 130, 3, 1
    shift = 3e-7
    assert fo.rung_of(shift)[0] == 0
    wins = [fo.lattice_window(kid, N, d, None, seed=1), fo.rung_window(kid, N, d, 70, seed=2, shift=shift)[:3],
            fo.lattice_window(kid, N, d, 100, seed=3)]
    X, y, theta = (np.stack([w[i] for w in wins]) for i in range(3))
    th10 = np.zeros((B, 10))
    th10[:, :theta.shape[1]] = theta

    def dev(*arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]

    def zeros(shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    def ladder_ok(info):   # host form: only the hopeless fit is left flagged
        assert info[0] == 0 and info[1] == 0 and info[2] == 101, info

    def noladder_ok(info):   # device form: no ladder, the jitter as given (none)
        assert info[0] == 0 and info[1] != 0 and info[2] == 101, info

    # multi-target: M = 17, P = 1 / 17 / 129, the engine's choice of the solve's tile height and both forced ones
    M = 17
    Xs = X[:, :M] + 0.25
    ctx = engine.Context(max_n=N, max_m=N, max_d=d, max_batch=B)
    assert ctx.multi_reserve(B, 129) == 0 and ctx.pgrad_reserve(B, N) == 0
    for P in (1, 17, 129):
        Y = np.stack([[fo._targets(N, 100 * b + p) for p in range(P)] for b in range(B)])
        Y[:, 0] = y
        dX, dY, dXs, dth = dev(X.transpose(0, 2, 1), Y, Xs.transpose(0, 2, 1), th10)
        for form in (0, 64, 128):
            assert ctx.multi_set_form(form) == 0
            res = ctx.fit_predict_multi_batch(X, Y, Xs, theta, kid)
            ladder_ok(res[4])
            out[f"fit_predict_multi_batch P{P} form{form}"] = flat(*res)
            dm, dv, dl, di = zeros((B, P, M)), zeros((B, M)), zeros((B, P)), zeros(B, torch.int32)
            assert ctx.fit_predict_multi_batch_device(B, N, d, M, P, kid, dX.data_ptr(), dY.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0,
                                                      True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
            torch.cuda.synchronize()
            res = [t.cpu().numpy() for t in (dm, dv, dl, di)]
            noladder_ok(res[3])
            out[f"fit_predict_multi_batch_device P{P} form{form}"] = flat(*res)
    assert ctx.multi_set_form(0) == 0

    # predictive gradients: M = 1 / 65 / 130
    for M in (1, 65, 130):
        Xs = X[:, :M] + 0.25
        res = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid)
        ladder_ok(res[4])
        out[f"fit_predict_grad_batch M{M}"] = flat(*res)
        dX, dy, dXs, dth = dev(X.transpose(0, 2, 1), y, Xs.transpose(0, 2, 1), th10)
        dm, dv, dl, di, dgm, dgv = zeros((B, M)), zeros((B, M)), zeros(B), zeros(B, torch.int32), zeros((B, M, d)), zeros((B, M, d))
        assert ctx.fit_predict_grad_batch_device(B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                                 dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(), dgm.data_ptr(),
                                                 dgv.data_ptr()) == 0
        torch.cuda.synchronize()
        res = [t.cpu().numpy() for t in (dm, dv, dl, di, dgm, dgv)]
        noladder_ok(res[3])
        out[f"fit_predict_grad_batch_device M{M}"] = flat(*res)
        for b in range(B):   # after a single fit: the ladder is cgp_fit's, the hopeless window leaves nothing to differentiate
            rc, logml = ctx.fit(X[b], y[b], kid, theta[b])
            assert (rc != 0) == (b == 2), (b, rc)
            out[f"predict_gradients M{M} fit {b}"] = flat(rc, logml, *(ctx.predict_gradients(Xs[b]) if rc == 0 else ()))
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


def window_calls(engine, out, sizes=(33, 64), kinds=((0, 1), (0, 3), (2, 1), (4, 1), (4, 3)), long_windows=True):
    W, S = 3, 3
    for N in sizes:
        for kid, d in kinds:
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

    if not long_windows:
        return
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


def window_host_calls(engine, out, sizes=(33, 64), kinds=((0, 1), (0, 3), (2, 1), (4, 1), (4, 3))):
    """Every window entry point of the host layer, host and device form, over the states of window_calls (empty, filling, origin
    moved, window 1 failed) at capacity 33 and 64: the pushes themselves (T = 1, N / 2, N + 5: the ring wraps), forecasts and
    predictive gradients at M = 1 / 20 / 70, the leave-one-out objective with and without logml, the optimisers capped at 12
    evaluations; on contexts of their own the multi-target family at P = 1 and 17 (two target tiles).  Then one push and one
    forecast of a capacity-528 window whose staged blocks pass 16 KiB (copied, not read in place)."""
    import torch
    W, S, EV = 3, 3, 12

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def zeros(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    def host(*ts):
        torch.cuda.synchronize()
        return flat(*[t.cpu().numpy() for t in ts])

    def guarded(f):   # a call that may be refused (the optimisers on a window whose theta is not positive)
        try:
            return flat(*[x for x in f() if x is not None])
        except engine.CgpError as e:
            return flat(e.code)

    def single_round(ctx, tag, Xs, xi, N, d, select):
        nth = ctx._win_nth
        for M in (1, 20, 70):
            xs = Xs[:, :M]
            out[f"window_predict {tag} M{M}"] = flat(*ctx.window_predict(xs, check=False))
            out[f"window_predict_gradients {tag} M{M}"] = flat(*ctx.window_predict_gradients(xs, check=False))
            out[f"window_predict_gradients dvar only {tag} M{M}"] = guarded(
                lambda: ctx.window_predict_gradients(xs, check=False, want=("dvar",), moments=()))
            dxs, m, v, gm, gv = dev(xs), zeros(W, M), zeros(W, M), zeros(W, M, d), zeros(W, M, d)
            assert ctx.window_predict_device(M, dxs.data_ptr(), True, m.data_ptr(), v.data_ptr()) == 0
            out[f"window_predict_device {tag} M{M}"] = host(m, v)
            assert ctx.window_predict_gradients_device(M, dxs.data_ptr(), False, m.data_ptr(), v.data_ptr(), gm.data_ptr(), gv.data_ptr()) == 0
            out[f"window_predict_gradients_device {tag} M{M}"] = host(m, v, gm, gv)
        M = 20
        dxs, dxi, m, cov, paths, info = dev(Xs[:, :M]), dev(xi[:, :, :M]), zeros(W, M), zeros(W, M, M), zeros(W, S, M), zeros(W, dtype=torch.int32)
        assert ctx.window_predict_cov_device(M, dxs.data_ptr(), True, m.data_ptr(), cov.data_ptr()) == 0
        assert ctx.window_sample_device(M, dxs.data_ptr(), S, dxi.data_ptr(), True, 1e-6, paths.data_ptr(), info.data_ptr()) == 0
        out[f"window_predict_cov_device window_sample_device {tag}"] = host(m, cov, paths, info)
        val, grad, lm = zeros(W), zeros(W, nth), zeros(W)
        for want in (True, False):
            out[f"window_loo_nll_grad logml {want} {tag}"] = guarded(lambda: ctx.window_loo_nll_grad(want_logml=want))
            assert ctx.window_loo_nll_grad_device(val.data_ptr(), grad.data_ptr(), nth, lm.data_ptr() if want else 0) == 0
            out[f"window_loo_nll_grad_device logml {want} {tag}"] = host(val, grad, lm)
        assert ctx.window_nll_grad_device(val.data_ptr(), grad.data_ptr(), nth) == 0
        out[f"window_nll_grad_device {tag}"] = host(val, grad)
        lo = [zeros(W, N) for _ in range(3)]
        assert ctx.window_loo_device(*[t.data_ptr() for t in lo], val.data_ptr()) == 0
        out[f"window_loo_device {tag}"] = host(*lo, val)
        out[f"window_optimize {tag}"] = guarded(lambda: ctx.window_optimize(max_evals=EV, select=select))
        out[f"window_optimize_loo {tag}"] = guarded(lambda: ctx.window_optimize_loo(max_evals=EV, select=select))

    def multi_round(ctx, tag, Xs, P, d, select):
        nth = ctx._win_nth
        for M in (1, 20):
            xs = Xs[:, :M]
            for want in (True, False):
                out[f"window_predict_multi logml {want} {tag} M{M}"] = guarded(lambda: ctx.window_predict_multi(xs, check=False, want_logml=want))
            dxs, m, v, lm = dev(xs), zeros(W, P, M), zeros(W, M), zeros(W, P)
            assert ctx.window_predict_multi_device(M, P, dxs.data_ptr(), False, m.data_ptr(), v.data_ptr(), lm.data_ptr()) == 0
            out[f"window_predict_multi_device {tag} M{M}"] = host(m, v, lm)
        val, grad, lm = zeros(W), zeros(W, nth), zeros(W, P)
        for want in (True, False):
            out[f"window_multi_nll_grad logml {want} {tag}"] = guarded(lambda: ctx.window_multi_nll_grad(want_logml=want))
            assert ctx.window_multi_nll_grad_device(P, val.data_ptr(), grad.data_ptr(), nth, lm.data_ptr() if want else 0) == 0
            out[f"window_multi_nll_grad_device logml {want} {tag}"] = host(val, grad, lm)
        out[f"window_optimize_multi {tag}"] = guarded(lambda: ctx.window_optimize_multi(max_evals=EV, select=select))

    def push_device(ctx, X, Y, P):   # (W, T, d), (W, T, P): the device form of the push, single-target when P is 0
        T = X.shape[1]
        dx, dy, pm, pv, lm = dev(X), dev(Y), zeros(W, T), zeros(W, T), zeros(W, T)
        if P:
            assert ctx.window_push_multi_device(T, P, dx.data_ptr(), dy.data_ptr(), True, pm.data_ptr(), pv.data_ptr(), lm.data_ptr()) == 0
        else:
            assert ctx.window_push_device(T, dx.data_ptr(), dy.data_ptr(), True, pm.data_ptr(), pv.data_ptr(), lm.data_ptr()) == 0
        return host(pm, pv, lm)

    for N in sizes:
        cuts = np.cumsum([0, 1, N // 2, N + 5, 2, 1])   # the pushes: T = 1, N / 2, N + 5, a device-form one of 2, one more after the failure
        for kid, d in kinds:
            for P in (0, 1, 17):   # 0: the single-target calls
                Xw, Yw = zip(*[window(cuts[-1], d, 10 * kid + N + d + w, kid, max(P, 1)) for w in range(W)])
                X, Y = np.stack(Xw), np.stack(Yw).transpose(0, 2, 1)   # (W, T, d), (W, T, P)
                rng = np.random.default_rng(N + kid + d)
                Xs = np.stack([points_for(kid, X[w, :N + 5], 70, rng) for w in range(W)])
                xi = rng.normal(size=(W, S, 70))
                theta = np.tile(theta_of(kid, d), (W, 1))
                ctx = engine.Context(max_n=8, max_m=8, max_d=d)
                ctx.window_init(W, N, d, kid, theta)
                if P:
                    assert ctx.window_multi_reserve(P) == 0 and ctx.window_multi_grad_reserve() == 0
                else:
                    assert ctx.window_joint_reserve(70) == 0 and ctx.window_loo_grad_reserve() == 0
                tag = f"kid{kid} N{N} d{d}" + (f" P{P}" if P else "")

                def push(i, check=True):
                    x, y = X[:, cuts[i]:cuts[i + 1]], Y[:, cuts[i]:cuts[i + 1]]
                    res = ctx.window_push_multi(x, y, check=check) if P else ctx.window_push(x, y[:, :, 0], check=check)
                    out[f"window_push{'_multi' if P else ''} {tag} T{x.shape[1]} from tick {cuts[i]}"] = flat(*res)

                def state(name, select=None):
                    if P:
                        multi_round(ctx, f"{tag} {name}", Xs, P, d, select)
                    else:
                        single_round(ctx, f"{tag} {name}", Xs, xi, N, d, select)

                state("empty")
                push(0)
                push(1)
                state("filling")
                push(2)
                state("origin moved")
                x, y = X[:, cuts[3]:cuts[4]], Y[:, cuts[3]:cuts[4]]
                out[f"window_push{'_multi' if P else ''}_device {tag}"] = push_device(ctx, x, y if P else y[:, :, 0], P)
                bad = theta.copy()
                bad[1, -1] = -2.0 * bad[1, 0]   # window 1's Ky is negative definite (window_calls)
                ctx.window_set_theta(bad, check=False)
                state("window 1 failed", select=[1, 0, 1])
                push(4, check=False)
                ctx.close()

    # staged blocks above 16 KiB: one window of capacity 528, a push of 600 ticks (28 KB) and a forecast at 600 points (19 KB)
    N, T, d, kid, M = 528, 600, 2, 1, 600
    X, Y = window(T, d, N + kid, kid)
    assert T * (d + 4) * 8 > 16 * 1024 and M * (d + 2) * 8 > 16 * 1024
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta_of(kid, d)[None])
    out[f"window_push by copy N{N} T{T}"] = flat(*ctx.window_push(X[None], Y[:1]))
    Xs = points_for(kid, X, M, np.random.default_rng(N))[None]
    out[f"window_predict by copy N{N} M{M}"] = flat(*ctx.window_predict(Xs))
    out[f"window_predict_gradients by copy N{N} M{M}"] = flat(*ctx.window_predict_gradients(Xs))
    ctx.close()


def run(out_path, windows_once=False):
    os.environ["CGP_SMALL"] = "off"
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, which has to be the process's first)
    import corenav_gp_amd.engine as engine
    engine.load()
    out = {}
    if windows_once:   # every window entry point at one shape: short enough to read as a launch listing under a kernel trace
        window_host_calls(engine, out, sizes=(33,), kinds=((4, 3),))
        window_calls(engine, out, sizes=(33,), kinds=((4, 3),), long_windows=False)
    else:
        batch_calls(engine, out)
        hooked_calls(engine, out)
        window_calls(engine, out)
        window_host_calls(engine, out)
    np.savez(out_path, **out)
    print(f"{len(out)} calls saved to {out_path} (library {engine.LIB_PATH})")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] in ("run", "run-windows-once"):
        run(sys.argv[2], sys.argv[1] != "run")
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
