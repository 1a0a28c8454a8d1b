"""GPU parity of the predictive gradients (cgp_fit_predict_grad_batch[_device], cgp_predict_gradients: d mean / d x* and
d var / d x* at M test points) against tests/pgrad_oracle.py, through the C ABI.  Bar: the project's fp64 bar, 1e-6, per fit
max|dmean - oracle| / max|oracle dmean| and the same for dvar.  The oracle itself sits at <= 7e-13 of a 50-digit restatement in
that metric (tests/test_oracle_pgrad.py) and the kernels measure <= 3e-12 (dmean) and <= 2.2e-9 (dvar, where its two terms
cancel) on the cases below: the bar tests the kernels, not the conditioning.  Windows and test points:
test_gpu_joint_batch.py's generator."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import failure_oracle as fo
import pgrad_oracle as po
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def window(N, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)]), y


def points_for(kid, X, M, rng):
    """RBF x Brownian: the reference's grid (the ticks after the last sample); else points around the window's last inputs."""
    if kid == 2:
        return X[-1, 0] + 1.0 + np.arange(M, dtype=np.float64)[:, None]
    N = len(X)
    return X[rng.integers(max(0, N - 50), N, size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def problem(B, N, d, M, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, yw = zip(*[window(N, d, seed + 17 * b, tick0=11 + b) for b in range(B)])
    X, y = np.stack(Xw), np.stack(yw)
    Xs = np.stack([points_for(kid, X[b], M, rng) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return X, y, Xs, theta, rng


def close(dmean, dvar, kid, theta, X, y, Xs, tol=TOL, what=""):
    odm, odv = po.predictive_gradients(po.fit(kid, theta, X, y), Xs)
    em = np.max(np.abs(dmean - odm)) / np.max(np.abs(odm))
    ev = np.max(np.abs(dvar - odv)) / np.max(np.abs(odv))
    print(f"{what} errors / bar: dmean {em / tol:.3g} dvar {ev / tol:.3g}")
    assert em <= tol and ev <= tol, (em, ev)


def ctx_for(engine, B, N, d, M, reserve_m=None, reserve_b=None, joint=False):
    ctx = engine.Context(max_n=N, max_m=max(M, reserve_m or 0), max_d=d, max_batch=B)
    assert ctx.pgrad_reserve(reserve_b or B, reserve_m or M) == 0
    if joint:
        assert ctx.joint_reserve(B, M) == 0
    return ctx


# N: 100 (one block step, no inner sum), 129 / 200 (two steps, partial last tile), 256 (no padding), 257 / 300 (three steps: a sum
# over two finished block columns, two hand-offs).  M + 1 at, below and above the 64- and 128-row tile edges, the z row alone in a
# tile (M = 128).  d = 1, 3, 8.  Every kernel id.
SHAPES = [(100, 1, 1, 0), (100, 16, 3, 1), (100, 127, 8, 4), (129, 15, 3, 3), (129, 130, 1, 2), (129, 64, 8, 1), (200, 63, 8, 1),
          (200, 64, 1, 4), (200, 128, 3, 0), (256, 127, 3, 0), (256, 128, 8, 4), (256, 1, 1, 2), (257, 130, 3, 1), (257, 16, 1, 2),
          (257, 63, 8, 3), (300, 63, 8, 3), (300, 128, 3, 1), (300, 1, 3, 4), (300, 15, 1, 0), (300, 127, 1, 2)]


@pytest.mark.parametrize("N,M,d,kid", SHAPES)
def test_shapes_and_kernels(engine, N, M, d, kid):
    B = 2
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 7 * N + M)
    Xc, yc, Xsc, thc = X.copy(), y.copy(), Xs.copy(), theta.copy()
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, var, logml, info, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid, include_noise=False)
    assert rc == 0 and not info.any() and dmean.shape == dvar.shape == (B, M, d)
    for b in range(B):
        close(dmean[b], dvar[b], kid, theta[b], X[b], y[b], Xs[b])
    assert np.array_equal(X, Xc) and np.array_equal(y, yc) and np.array_equal(Xs, Xsc) and np.array_equal(theta, thc)
    if N > 160:   # a tiled shape for the marginal call too: bitwise its outputs
        rc, pm, pv, plm, _ = ctx.fit_predict_batch(X, y, Xs, theta, kid, include_noise=False)
        assert np.array_equal(mean, pm) and np.array_equal(var, pv) and np.array_equal(logml, plm)
    # include_noise does not enter
    rc, _, var2, _, _, dmean2, dvar2 = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid, include_noise=True)
    assert rc == 0 and np.array_equal(dmean, dmean2) and np.array_equal(dvar, dvar2) and not np.array_equal(var, var2)


def test_reference_work_item_and_points_inside_the_window(engine):
    """N = 134, RBF x Brownian, M = 599 on the tick grid after the window (the reference's own request); then points inside the
    window, on the ticks (ties |x*| = |x_i|: the bracket is 0) and off them."""
    t, s = synth.reference_window()
    _, _, xtr, ytr = go.slip_node_split(t, s)
    X, y = xtr, ytr[:, 0]
    N = len(y)
    theta = np.array([0.5, 30.0, 0.01, 0.002])
    grid = points_for(2, X, 599, None)
    M = len(grid)
    assert M == 599 and N == 134
    ctx = ctx_for(engine, 1, N, 1, M)
    rc, mean, var, _, info, dmean, dvar = ctx.fit_predict_grad_batch(X[None], y[None], grid[None], theta[None], 2)
    assert rc == 0 and info[0] == 0
    close(dmean[0], dvar[0], 2, theta, X, y, grid, what="tick grid")
    rng = np.random.default_rng(5)
    inside = np.concatenate([X[rng.integers(0, N, size=40), 0], X[rng.integers(0, N - 1, size=40), 0] + rng.uniform(0.1, 0.9, size=40)])
    inside = inside[:, None]
    rc, _, _, _, _, dm, dv = ctx.fit_predict_grad_batch(X[None], y[None], inside[None], theta[None], 2)
    assert rc == 0
    close(dm[0], dv[0], 2, theta, X, y, inside, what="inside")


@pytest.mark.parametrize("B", [1, 64, 200, 512])
def test_every_schedule(engine, B):
    """N = 257, M = 17 through the latency, mid-size, fused and split schedules: some fits against the oracle; mean / var / logml
    bitwise the marginal call's; a fit's gradients do not depend on its slot or its neighbours (the same call, rotated)."""
    N, d, M, kid = 257, 3, 17, 1
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 2000 + B)
    ctx = ctx_for(engine, B, N, d, M)
    rc, mean, var, logml, info, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid)
    assert rc == 0 and not info.any()
    rc, pm, pv, plm, _ = ctx.fit_predict_batch(X, y, Xs, theta, kid)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv) and np.array_equal(logml, plm)
    for b in sorted({0, B // 2, B - 1}):
        close(dmean[b], dvar[b], kid, theta[b], X[b], y[b], Xs[b])
    if B > 1:
        perm = np.roll(np.arange(B), 5)
        perm[[0, 1]] = perm[[1, 0]]
        rc, _, _, _, _, rdm, rdv = ctx.fit_predict_grad_batch(X[perm], y[perm], Xs[perm], theta[perm], kid)
        assert rc == 0 and np.array_equal(rdm, dmean[perm]) and np.array_equal(rdv, dvar[perm])


def device_arrays(torch, X, y, Xs, theta):
    B = X.shape[0]
    th = np.zeros((B, 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, Xs.transpose(0, 2, 1), th)]


@pytest.mark.parametrize("B,N", [(3, 300), (60, 257)])
def test_host_device_and_graph_replay_agree_bitwise(engine, B, N):
    import torch
    d, M, kid = 3, 53, 1
    X, y, Xs, theta, rng = problem(B, N, d, M, kid, 9 + B)
    ctx = ctx_for(engine, B, N, d, M, reserve_m=64)
    rc, mean, var, logml, _, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid)
    assert rc == 0
    dX, dy, dXs, dth = device_arrays(torch, X, y, Xs, theta)
    dm = torch.empty((B, M), dtype=torch.float64, device="cuda")
    dv = torch.empty((B, M), dtype=torch.float64, device="cuda")
    dl = torch.empty(B, dtype=torch.float64, device="cuda")
    di = torch.empty(B, dtype=torch.int32, device="cuda")
    gm = torch.empty((B, M, d), dtype=torch.float64, device="cuda")
    gv = torch.empty((B, M, d), dtype=torch.float64, device="cuda")
    args = (B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0)

    def clear():
        for t in (dm, dv, dl, gm, gv):
            t.fill_(-1.0)
        di.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dv.cpu().numpy(), var)
        assert np.array_equal(dl.cpu().numpy(), logml) and not di.cpu().numpy().any()
        assert np.array_equal(gm.cpu().numpy(), dmean) and np.array_equal(gv.cpu().numpy(), dvar)

    def enqueue(s):
        assert ctx.fit_predict_grad_batch_device(*args, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(),
                                                 gm.data_ptr(), gv.data_ptr(), stream=s) == 0

    for stream_arg in (0, engine.STREAM_CTX):
        clear()
        enqueue(stream_arg)
        check()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        clear()
        graph.replay()
        check()
    # one gradient alone: the other buffer is not touched
    clear()
    assert ctx.fit_predict_grad_batch_device(*args, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(), 0, gv.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(gv.cpu().numpy(), dvar) and np.all(gm.cpu().numpy() == -1.0)


def test_device_form_failed_fit_is_nan_neighbours_are_bitwise(engine):
    """tests/failure_oracle.py's lattice: fit 1 has a duplicated input and a negative shift, jitter 0 (no ladder in the device
    form): its status word is the failing pivot, its gradients are NaN; fits 0 and 2 are bitwise what a call without the failing
    fit gives (the good lattice window in slot 1)."""
    import torch
    B, N, d, M, kid = 3, fo.N_TILED, fo.D_TILED, fo.M_TILED, 1
    good = fo.lattice_window(kid, N, d, None, seed=1)
    bad = fo.lattice_window(kid, N, d, 192, 96, seed=1)
    rng = np.random.default_rng(4)
    Xs = np.stack([good[0][rng.integers(0, N, size=M)] + 0.2 * rng.normal(size=(M, d)) for _ in range(B)])
    outs = []
    ctx = ctx_for(engine, B, N, d, M)
    for mid in (bad, good):
        X = np.stack([good[0], mid[0], good[0]])
        y = np.stack([good[1], mid[1], fo._targets(N, 2)])
        theta = np.stack([good[2], mid[2], good[2]])
        dX, dy, dXs, dth = device_arrays(torch, X, y, Xs, theta)
        dm = torch.zeros((B, M), dtype=torch.float64, device="cuda")
        dv = torch.zeros((B, M), dtype=torch.float64, device="cuda")
        dl = torch.zeros(B, dtype=torch.float64, device="cuda")
        di = torch.zeros(B, dtype=torch.int32, device="cuda")
        gm = torch.zeros((B, M, d), dtype=torch.float64, device="cuda")
        gv = torch.zeros((B, M, d), dtype=torch.float64, device="cuda")
        assert ctx.fit_predict_grad_batch_device(B, N, d, M, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, False,
                                                 dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr(), gm.data_ptr(),
                                                 gv.data_ptr()) == 0
        torch.cuda.synchronize()
        outs.append((di.cpu().numpy(), gm.cpu().numpy(), gv.cpu().numpy(), X, y, theta))
    info, gm, gv, X, y, theta = outs[0]
    assert info[1] == 193 and info[0] == 0 and info[2] == 0
    assert np.all(np.isnan(gm[1])) and np.all(np.isnan(gv[1]))
    ginfo, ggm, ggv = outs[1][:3]
    assert not ginfo.any()
    for b in (0, 2):
        assert np.array_equal(gm[b], ggm[b]) and np.array_equal(gv[b], ggv[b])
        close(gm[b], gv[b], kid, theta[b], X[b], y[b], Xs[b])
    close(ggm[1], ggv[1], kid, good[2], good[0], good[1], Xs[1])


def test_host_form_ladder_repairs_the_fit_from_slab_0(engine):
    """Fit 1 needs the ladder's rung k = 2 (failure_oracle.rung_window): it is re-submitted as a call of one, its factor lands in
    slab 0 and its gradients in slot 1 -- they meet the oracle's refit at the same jitter; fits 0 and 2 are bitwise what they are
    without the bad neighbour."""
    B, N, d, M, kid = 3, fo.N_TILED, fo.D_TILED, fo.M_TILED, 1
    good = fo.lattice_window(kid, N, d, None, seed=1, shift=3e-5)
    Xb, yb, thb, k, jit = fo.rung_window(kid, N, d, 192, 96, seed=1)
    rng = np.random.default_rng(6)
    Xs = np.stack([good[0][rng.integers(0, N, size=M)] + 0.2 * rng.normal(size=(M, d)) for _ in range(B)])
    ctx = ctx_for(engine, B, N, d, M)
    X, y, theta = np.stack([good[0], Xb, good[0]]), np.stack([good[1], yb, fo._targets(N, 2)]), np.stack([good[2], thb, good[2]])
    rc, mean, var, logml, info, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid, include_noise=False)
    assert rc == 0 and not info.any()
    f1 = po.fit(kid, thb, Xb, yb)
    assert f1.jitter > 0
    for b in range(B):
        close(dmean[b], dvar[b], kid, theta[b], X[b], y[b], Xs[b], what=f"fit {b}")
    Xg, yg, thg = X.copy(), y.copy(), theta.copy()
    Xg[1], yg[1], thg[1] = good
    rc, _, _, _, _, gdm, gdv = ctx.fit_predict_grad_batch(Xg, yg, Xs, thg, kid, include_noise=False)
    assert rc == 0
    for b in (0, 2):
        assert np.array_equal(dmean[b], gdm[b]) and np.array_equal(dvar[b], gdv[b])


def test_joint_covariance_is_the_same_after_a_gradient_call(engine):
    """The backward solve leaves V^T in the panel: cgp_predict_cov before and after cgp_predict_gradients, bitwise; and
    predict_gradients' mean / var are bitwise cgp_predict's; factor and alpha of the resident fit are untouched."""
    N, d, M, kid = 300, 3, 70, 4
    X, y, Xs, theta, rng = problem(1, N, d, M, kid, 12)
    ctx = ctx_for(engine, 1, N, d, M, joint=True)
    assert ctx.fit(X[0], y[0], kid, theta[0])[0] == 0
    L0, a0 = ctx.factor(), ctx.alpha()
    m0, c0 = ctx.predict_cov(Xs[0], include_noise=False)
    pm, pv = ctx.predict(Xs[0], include_noise=False)
    mean, var, dmean, dvar = ctx.predict_gradients(Xs[0])
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    close(dmean, dvar, kid, theta[0], X[0], y[0], Xs[0])
    m1, c1 = ctx.predict_cov(Xs[0], include_noise=False)
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(L0, ctx.factor()) and np.array_equal(a0, ctx.alpha())
    # fewer points than reserved, after a larger call
    mean, var, dm3, dv3 = ctx.predict_gradients(Xs[0][:3])
    assert np.array_equal(dm3, dmean[:3]) and np.array_equal(dv3, dvar[:3])
    # the batch form: the covariance call right after a gradient call of the same fits
    rc, _, cb, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=False)
    rc2 = ctx.fit_predict_grad_batch(X, y, Xs, theta, kid, include_noise=False)[0]
    rc3, _, ca, _, _ = ctx.fit_predict_cov_batch(X, y, Xs, theta, kid, include_noise=False)
    assert rc == rc2 == rc3 == 0 and np.array_equal(cb, ca)


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.zeros(256)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 8, 1, 4, 2)   # batch, N, d, M, kernel

    def host(h=ctx.h, shape=shape, dm=p, dv=p, mean=p):
        return lib.cgp_fit_predict_grad_batch(h, *shape, p, p, p, p, 4, 1, mean, p, p, ip, dm, dv)

    def dev(h=ctx.h, shape=shape, dm=a, dv=a):
        return lib.cgp_fit_predict_grad_batch_device(h, *shape, a, a, a, a, None, 1, a, a, a, a, dm, dv, None)

    def single(h=ctx.h, M=4, dm=p, dv=p):
        return lib.cgp_predict_gradients(h, p, M, p, p, dm, dv)

    assert host() == ESTATE and dev() == ESTATE and single() == ESTATE        # no reservation
    # the order of the answers: no context and M = 0 before the missing reservation ...
    assert host(h=None) == EINVAL and dev(h=None) == EINVAL and single(h=None) == EINVAL and lib.cgp_pgrad_reserve(None, 1, 4) == EINVAL
    assert host(shape=(1, 9, 1, 0, 2)) == EINVAL and dev(shape=(1, 9, 1, 0, 2)) == EINVAL and single(M=0) == EINVAL
    for mb, mm in ((0, 4), (3, 4), (1, 0), (1, 9)):
        assert lib.cgp_pgrad_reserve(ctx.h, mb, mm) == EINVAL
    assert lib.cgp_pgrad_reserve(ctx.h, 1, 4) == 0
    assert single() == ESTATE                                                  # reserved, but nothing fitted
    for s in ((1, 8, 1, 5, 2), (2, 8, 1, 4, 2)):
        assert host(shape=s) == ECAPACITY and dev(shape=s) == ECAPACITY
    assert single(M=5) == ECAPACITY
    for s in ((2, 9, 1, 1, 2), (1, 9, 1, 5, 2)):                               # ... the capacity before the arrays
        assert host(shape=s, dm=None, dv=None) == ECAPACITY and host(shape=s, mean=None) == ECAPACITY
        assert dev(shape=s, dm=None, dv=None) == ECAPACITY
    assert single(M=5, dm=None, dv=None) == ECAPACITY
    m0 = (1, 8, 1, 0, 2)
    assert host(shape=m0) == EINVAL and dev(shape=m0) == EINVAL and single(M=0) == EINVAL
    assert host(dm=None, dv=None) == EINVAL and dev(dm=None, dv=None) == EINVAL and single(dm=None, dv=None) == EINVAL
    assert host(mean=None) == EINVAL
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_pgrad_reserve(f32.h, 1, 4) == EINVAL
    assert host(h=f32.h) == EINVAL and dev(h=f32.h) == EINVAL and single(h=f32.h) == EINVAL
    # both contexts are still usable
    X, y, Xs, theta, rng = problem(1, 8, 1, 4, 2, 1)
    rc, _, _, _, info, dmean, dvar = ctx.fit_predict_grad_batch(X, y, Xs, theta, 2)
    assert rc == 0 and info[0] == 0
    close(dmean[0], dvar[0], 2, theta[0], X[0], y[0], Xs[0])
    rc, m32, _, _, _ = f32.fit_predict_batch(X, y, Xs, theta, 2)
    assert rc == 0 and np.all(np.isfinite(m32))
