"""GPU parity of the sparse fits' objective (cgp_sparse_nll_grad_batch[_device], cgp_optimize_sparse_batch: the gradient of the
collapsed variational bound in theta and in the inducing inputs Z, and its L-BFGS; include/corenav_gp.h) against
tests/sparse_grad_oracle.py, through engine.py.  Bars: 1e-6 against the oracle -- nll against max(1, |nll|), grad and gradZ each
against its block's largest |component| in the oracle -- and bitwise wherever the header promises it.  Every input that is compared
meets sparse_oracle.conditions_hold and agrees with central differences of the oracle's bound: asserted for the whole list COMPARED
on the CPU by test_oracle_sparse_grad.py, which imports the generators below.  Shapes sit on the kernels' edges: m across the
16-row tiles and across the groups of eight row tiles of k_sparse_grad_panel (128 | 129), N across its sub-panels and chunks."""
import os

import numpy as np
import pytest

import sparse_oracle as so
import sparse_grad_oracle as sg
import test_gpu_sparse as tg

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1
CHUNK = tg.CHUNK
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_sparse_grad.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def problem(B, N, d, m, kid, seed, spacing=tg.SPACING):
    """test_gpu_sparse.problem without test points; spacing: the lattice of the inducing inputs, in length-scales (a shape whose
    K_uu cannot meet the conditions at 1.25 is spread wider: such a case tests indexing, not conditioning)."""
    old = tg.SPACING
    tg.SPACING = spacing
    try:
        X, y, Z, _, theta = tg.problem(B, N, d, 0, m, kid, seed)
    finally:
        tg.SPACING = old
    return X, y, Z, theta


def history(N, m, seed):
    X, y, Z, _, theta = tg.history(N, m, 0, seed)
    return X, y, Z, theta


def golden(kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_grad_mp_k{kid}.npz"))
    return g["X"][None], g["y"][None], g["Z"][None], g["theta"][None]


EVERY_KERNEL = tg.EVERY_KERNEL
M_IND_EDGES = [1, 15, 16, 17, 127, 128, 129, 512]      # 128 | 129: one | two groups of row tiles in k_sparse_grad_panel
N_EDGES = [1, 3, 17, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
S8 = (2, 40, 8, 512, 1, 77, 2.5)                       # sparse_shape picks S = 8: the panel and Z do not fit LDS at S = 16
HISTORY = (20000, 48, 3)
OPT_THETA = [0, 1, 2, 4]
OPT_JOINT = [1, 4]
# every (generator, arguments, fit, kernel) compared with the oracle: test_oracle_sparse_grad.py asserts the conditions on each
COMPARED = ([("problem", (2, 130, d, 17, kid, 10 * kid + d), b, kid) for kid, d in EVERY_KERNEL for b in (0, 1)]
            + [("problem", (2, 130, 2, m, 1, 100 + m), 1, 1) for m in M_IND_EDGES]
            + [("problem", (2, N, 2, 17, 1, 200 + N), 1, 1) for N in N_EDGES]
            + [("problem", S8, 1, 1)]
            + [("problem", (2, 5, 2, 17, 1, 300), 1, 1)]
            + [("problem", (2, 130, 1, 33, 2, 310), 0, 2), ("problem", (2, 700, 3, 70, 3, 320), 1, 3)]
            + [("history", HISTORY, 0, 0)]
            + [("problem", (3, 200, 2, 40, 1, 9), b, 1) for b in (0, 2)]
            + [("golden", (kid,), 0, kid) for kid in range(5)])


def extent(shape, kid):
    """test_gpu_sparse.EXTENT_CASES' inputs (test_gpu_sparse_grad_extents.py), without the test points."""
    X, y, Z, _, theta = tg.problem(*tg.extent_args(shape, kid))
    return X, y, Z, theta


COMPARED += [("extent", (shape, kid), 1, kid) for shape, kid in tg.EXTENT_CASES] + [("problem", (1, 40, 1, 3, 2, 2), 0, 2)]


def generate(name, args):
    return {"problem": problem, "history": history, "golden": golden, "extent": extent}[name](*args)


def opt_problem(kid):
    d = 1 if kid == 2 else 3
    X, y, Z, theta = problem(1, 130, d, 17, kid, 500 + kid)
    return X, y, Z, theta


def ctx_for(engine, B, N, d, m):
    ctx = engine.Context(max_n=16, max_m=8, max_d=d, max_batch=B)
    assert ctx.sparse_reserve(B, N, m, 8) == 0 and ctx.sparse_grad_reserve(B) == 0
    return ctx


def errors(nll, g, gz, onll, og, ogz):
    e = [abs(nll - onll) / max(1.0, abs(onll)), np.max(np.abs(g - og)) / np.max(np.abs(og))]
    if gz is not None:
        e.append(np.max(np.abs(gz - ogz)) / np.max(np.abs(ogz)))
    return [float(v) for v in e]


def close(kid, theta, X, y, Z, nll, g, gz, jitter=0.0, need_conditions=True):
    if need_conditions:
        o = so.fit_predict_sparse(kid, theta, X, y, Z, None)
        assert so.conditions_hold(o), (o.info, o.ladder, o.cond_uu, o.cond_b)
    onll, og, ogz, info = sg.nll_grad(kid, theta, X, y, Z, jitter=jitter)
    assert info == 0
    e = errors(nll, g, gz, onll, og, ogz)
    for k, v in zip(("nll", "grad", "gradZ"), e):
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("errors / bar: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in zip(("nll", "grad", "gradZ"), e)))
    assert max(e) <= TOL, e


def run_and_compare(engine, name, args, kid, fits):
    X, y, Z, theta = generate(name, args)
    B, N, d = X.shape
    m = Z.shape[1]
    ctx = ctx_for(engine, B, N, d, m)
    rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)
    assert rc == 0 and not info.any()
    assert nll.shape == (B,) and g.shape == theta.shape and gz.shape == Z.shape
    for b in fits:
        close(kid, theta[b], X[b], y[b], Z[b], nll[b], g[b], gz[b])
    return ctx, (X, y, Z, theta), (nll, g, gz)


@pytest.mark.parametrize("kid,d", EVERY_KERNEL)
def test_every_kernel(engine, kid, d):
    run_and_compare(engine, "problem", (2, 130, d, 17, kid, 10 * kid + d), kid, (0, 1))


@pytest.mark.parametrize("kid", range(5))
def test_fifty_digit_pins(engine, kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_grad_mp_k{kid}.npz"))
    X, y, Z, theta = golden(kid)
    ctx = ctx_for(engine, 1, X.shape[1], X.shape[2], Z.shape[1])
    rc, nll, gr, gz, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)
    assert rc == 0 and not info.any()
    e = errors(nll[0], gr[0], gz[0], -float(g["bound"]), g["grad"], g["gradZ"])
    print("errors / 1e-6 against the 50-digit dense statement:", [v / TOL for v in e])
    assert max(e) <= TOL, e


@pytest.mark.parametrize("m", M_IND_EDGES)
def test_inducing_edges(engine, m):
    run_and_compare(engine, "problem", (2, 130, 2, m, 1, 100 + m), 1, (1,))


@pytest.mark.parametrize("N", N_EDGES)
def test_sample_edges(engine, N):
    assert engine.load().cgp_sparse_chunk() == CHUNK
    run_and_compare(engine, "problem", (2, N, 2, 17, 1, 200 + N), 1, (1,))


def test_half_width_sub_panels(engine):
    run_and_compare(engine, "problem", S8, 1, (1,))


def test_fewer_samples_than_inducing_inputs(engine):
    run_and_compare(engine, "problem", (2, 5, 2, 17, 1, 300), 1, (1,))


def test_other_kernels_across_tiles(engine):
    run_and_compare(engine, "problem", (2, 130, 1, 33, 2, 310), 2, (0,))
    run_and_compare(engine, "problem", (2, 700, 3, 70, 3, 320), 3, (1,))


def test_history_beyond_the_context(engine):
    run_and_compare(engine, "history", HISTORY, 0, (0,))


def device_arrays(torch, X, y, Z, theta):
    th = np.zeros((X.shape[0], 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, Z.transpose(0, 2, 1), th)]


def device_outputs(torch, B, d, m, fill=-1.0):
    f = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    return f(B), f(B, 10), f(B, d, m), torch.full((B,), -1, dtype=torch.int32, device="cuda")


def test_slot_batch_and_neighbours_do_not_move_a_fit(engine):
    B, N, d, m, kid = 3, 200, 2, 40, 1
    X, y, Z, theta = problem(B, N, d, m, kid, 9)
    alone = ctx_for(engine, 1, N, d, m).sparse_nll_grad_batch(X[:1], y[:1], Z[:1], theta[:1], kid)
    assert alone[0] == 0
    ctx = ctx_for(engine, B, N, d, m)
    for order in ([0, 1, 2], [1, 2, 0]):
        rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X[order], y[order], Z[order], theta[order], kid)
        assert rc == 0 and not info.any()
        s = order.index(0)
        assert nll[s] == alone[1][0] and np.array_equal(g[s], alone[2][0]) and np.array_equal(gz[s], alone[3][0])
    close(kid, theta[0], X[0], y[0], Z[0], alone[1][0], alone[2][0], alone[3][0])


def test_host_device_and_graph_replay_agree_bitwise_and_nll_is_minus_the_bound(engine):
    import torch
    B, N, d, m, kid = 2, 700, 3, 70, 1
    X, y, Z, theta = problem(B, N, d, m, kid, 10)
    ctx = ctx_for(engine, B, N, d, m)
    rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)
    assert rc == 0 and not info.any()
    rc, nll0, g0, none, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid, want_grad_z=False)
    assert rc == 0 and none is None and np.array_equal(nll0, nll) and np.array_equal(g0, g)   # grad with and without gradZ
    dX, dy, dZ, dth = device_arrays(torch, X, y, Z, theta)
    dn, dg, dgz, di = device_outputs(torch, B, d, m)

    def clear():
        for t in (dn, dg, dgz):
            t.fill_(-1.0)
        di.fill_(-1)
        torch.cuda.synchronize()

    def check(with_z=True):
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dn.cpu().numpy(), nll) and np.array_equal(dg.cpu().numpy()[:, :theta.shape[1]], g)
        assert np.all(dg.cpu().numpy()[:, theta.shape[1]:] == -1.0) and not di.cpu().numpy().any()
        if with_z:
            assert np.array_equal(dgz.cpu().numpy().transpose(0, 2, 1), gz)
        else:
            assert np.all(dgz.cpu().numpy() == -1.0)

    def enqueue(stream, with_z=True):
        assert ctx.sparse_nll_grad_batch_device(B, N, d, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0,
                                                dn.data_ptr(), dg.data_ptr(), 10, dgz.data_ptr() if with_z else 0, di.data_ptr(),
                                                stream) == 0

    clear()
    enqueue(0)
    check()
    clear()
    enqueue(0, with_z=False)
    check(with_z=False)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    clear()
    graph.replay()
    check()
    # nll = -bound of the forward call, bitwise, for M = 0 and M > 0; and the forward call is what it is without the gradient call
    Xs = np.ascontiguousarray(X[:, :19])
    fresh = ctx_for(engine, B, N, d, m)
    assert fresh.sparse_reserve(B, N, m, 19) == 0
    before = fresh.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    assert ctx.sparse_reserve(B, N, m, 19) == 0
    after = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    only = ctx.fit_predict_sparse_batch(X, y, Z, None, theta, kid)
    assert before[0] == 0 and after[0] == 0 and only[0] == 0
    for a, b in zip(before[1:], after[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(-after[3], nll) and np.array_equal(-only[3], nll)
    rc, nll2, g2, gz2, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)   # ... and the gradient call after a forward call
    assert rc == 0 and np.array_equal(nll2, nll) and np.array_equal(g2, g) and np.array_equal(gz2, gz)


def test_scratch_left_full_of_nan_by_another_shape_does_not_move_a_call(engine):
    B, N, d, m, kid = 2, 300, 2, 33, 1
    X, y, Z, theta = problem(B, N, d, m, kid, 12)
    fresh = ctx_for(engine, B, N, d, m).sparse_nll_grad_batch(X, y, Z, theta, kid)
    ctx = ctx_for(engine, B, 1100, d, 100)
    X2, y2, Z2, th2 = problem(B, 1100, d, 100, kid, 13)
    y2[:] = np.nan   # K_uu and B factor, and NaN runs through every scratch section the next call uses
    rc, nll2, g2, gz2, info2 = ctx.sparse_nll_grad_batch(X2, y2, Z2, th2, kid)
    assert np.all(np.isnan(nll2)) and np.all(np.isnan(g2)) and np.all(np.isnan(gz2))
    again = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)
    assert again[0] == 0 and fresh[0] == 0
    for a, f in zip(again[1:], fresh[1:]):
        assert np.array_equal(a, f)


def test_failed_fit_is_nan_with_its_pivot_and_the_neighbours_are_untouched(engine):
    B, N, d, m, kid = 3, 200, 2, 40, 1
    X, y, Z, theta = problem(B, N, d, m, kid, 9)
    ctx = ctx_for(engine, B, N, d, m)
    alone = {b: ctx.sparse_nll_grad_batch(X[b:b + 1], y[b:b + 1], Z[b:b + 1], theta[b:b + 1], kid) for b in (0, 2)}
    Zn = Z.copy()
    Zn[1, 1, 0] = np.nan   # beyond every step of the ladder
    rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X, y, Zn, theta, kid)
    assert 1 <= rc <= m and list(info) == [0, rc, 0]
    assert np.isnan(nll[1]) and np.all(np.isnan(g[1])) and np.all(np.isnan(gz[1]))
    for b in (0, 2):
        assert nll[b] == alone[b][1][0] and np.array_equal(g[b], alone[b][2][0]) and np.array_equal(gz[b], alone[b][3][0])


def test_host_form_climbs_the_ladder_on_identical_inducing_inputs(engine):
    X, y, Z, Xs, theta, kid = tg.failing_problem()
    B, N, d = X.shape
    m = Z.shape[1]
    ctx = ctx_for(engine, B, N, d, m)
    rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, kid)
    assert rc == 0 and not info.any()
    onll, og, ogz, oinfo, steps, jit = sg.nll_grad_ladder(kid, theta[1], X[1], y[1], Z[1])
    assert oinfo == 0 and steps == 1
    e = errors(nll[1], g[1], gz[1], onll, og, ogz)
    print(f"ladder step 1, jitter {jit:.3g}; errors / 1e-6: {[v / TOL for v in e]}")
    assert max(e) <= TOL, e


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.ones(512)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 40, 1, 3, 2)   # batch, N, d, m, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, z=p, th=p, stride=4, nll=p, grad=p, gstride=4, gz=p):
        return lib.cgp_sparse_nll_grad_batch(h, *shape, x, y, z, th, stride, nll, grad, gstride, gz, ip)

    def dev(h=ctx.h, shape=shape, x=a, y=a, z=a, th=a, nll=a, grad=a, gstride=4, gz=a, info=a):
        return lib.cgp_sparse_nll_grad_batch_device(h, *shape, x, y, z, th, None, nll, grad, gstride, gz, info, None)

    def opt(h=ctx.h, shape=shape, x=p, y=p, z=p, th=p, stride=4):
        return lib.cgp_optimize_sparse_batch(h, *shape, x, y, z, th, stride, 1, 5, None, None)

    calls = (host, dev, opt)
    assert all(f() == ESTATE for f in calls)                                      # no reservation at all
    assert lib.cgp_sparse_grad_reserve(ctx.h, 1) == ESTATE                        # ... nor can there be one of this section's
    for f in calls:                                                               # no context and the counts come first
        assert f(h=None) == EINVAL
        for s in ((0, 40, 1, 3, 2), (1, 0, 1, 3, 2), (1, 40, 0, 3, 2), (1, 40, 1, 0, 2), (1, 40, 1, 513, 2), (1, 40, 1, 3, 5),
                  (1, 40, 1, 3, -1)):
            assert f(shape=s) == EINVAL, s
    assert lib.cgp_sparse_reserve(ctx.h, 1, 40, 3, 4) == 0
    assert all(f() == ESTATE for f in calls)                                      # the sparse reservation alone is not enough
    assert lib.cgp_sparse_grad_reserve(None, 1) == EINVAL
    for mb in (0, 3):
        assert lib.cgp_sparse_grad_reserve(ctx.h, mb) == EINVAL
    assert lib.cgp_sparse_grad_reserve(ctx.h, 2) == ESTATE                        # beyond the sparse reservation's batch
    assert lib.cgp_sparse_grad_reserve(ctx.h, 1) == 0
    for f in calls:
        for s in ((2, 40, 1, 3, 2), (1, 41, 1, 3, 2), (1, 40, 1, 4, 2), (1, 40, 2, 3, 1)):
            assert f(shape=s) == ECAPACITY, s                                     # batch, N, m, d beyond the reservations / context
            assert f(shape=s, x=None) == ECAPACITY                                # ... before the arrays
        assert f(shape=(1, 40, 2, 3, 2)) == EINVAL                                # RBF x Brownian needs d = 1
    for k in ("x", "y", "z", "th", "nll", "grad"):
        assert host(**{k: None}) == EINVAL, k
    assert host(stride=3) == EINVAL and host(gstride=3) == EINVAL
    for k in ("x", "y", "z", "th", "nll", "grad", "info"):
        assert dev(**{k: None}) == EINVAL, k
    assert dev(gstride=3) == EINVAL
    for k in ("x", "y", "z", "th"):
        assert opt(**{k: None}) == EINVAL, k
    assert opt(stride=3) == EINVAL
    zero = np.ones(512)
    zero[1] = 0.0
    assert opt(th=engine._p(zero)) == EINVAL                                      # a theta <= 0
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_sparse_grad_reserve(f32.h, 1) == EINVAL and all(f(h=f32.h) == EINVAL for f in calls)
    # a later, larger sparse reservation does not widen this one
    assert lib.cgp_sparse_reserve(ctx.h, 1, 80, 3, 4) == 0
    assert host(shape=(1, 80, 1, 3, 2)) == ECAPACITY
    # the context is still usable; gradZ and info may be NULL in the host form
    X, y, Z, theta = problem(1, 40, 1, 3, 2, 2)
    assert lib.cgp_sparse_nll_grad_batch(ctx.h, 1, 40, 1, 3, 2, engine._p(X), engine._p(y), engine._p(Z), engine._p(theta), 4, p,
                                         engine._p(zero), 4, None, None) == 0
    rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(X, y, Z, theta, 2)
    assert rc == 0 and nll[0] == buf[0] and np.array_equal(g[0], zero[:4])
    close(2, theta[0], X[0], y[0], Z[0], nll[0], g[0], gz[0])


def test_symbols_exported(engine):
    for name in ("cgp_sparse_grad_reserve", "cgp_sparse_nll_grad_batch", "cgp_sparse_nll_grad_batch_device", "cgp_optimize_sparse_batch"):
        assert name in engine.EXPORTS and hasattr(engine.load(), name)


# ---- optimiser ---------------------------------------------------------------------------------------------------
_SCIPY = {}


def scipy_run(kid, optimize_z, factr=1e7):
    """scipy on the oracle from the optimiser tests' start, computed once per (kernel, mode, factr)."""
    key = (kid, optimize_z, factr)
    if key not in _SCIPY:
        X, y, Z, theta = opt_problem(kid)
        _SCIPY[key] = sg.optimize_sparse(kid, X[0], y[0], Z[0], theta[0], optimize_z, factr=factr)
    return _SCIPY[key]


def run_optimiser(engine, kid, optimize_z):
    X, y, Z, theta = opt_problem(kid)
    B, N, d = X.shape
    m = Z.shape[1]
    ctx = ctx_for(engine, B, N, d, m)
    th, Zr, bound, nev = ctx.optimize_sparse_batch(X, y, Z, theta, kid, optimize_z=optimize_z)
    assert np.all(th > 0) and (optimize_z or np.array_equal(Zr, Z))
    # the bound a fresh forward call returns at the returned point, bitwise
    rc, _, _, again, info = ctx.fit_predict_sparse_batch(X, y, Zr, None, th, kid)
    assert rc == 0 and not info.any() and np.array_equal(again, bound)
    return ctx, th, Zr, bound, nev


@pytest.mark.parametrize("kid", OPT_THETA)
def test_optimiser_over_theta_reaches_scipys_bound(engine, kid):
    _, th, Zr, bound, nev = run_optimiser(engine, kid, False)
    sth, sZ, sbound, sev, warn, ladders = scipy_run(kid, False)
    assert warn == 0 and ladders == 0
    rel = abs(bound[0] - sbound) / max(1.0, abs(sbound))
    print(f"kernel {kid}: bound {bound[0]:.9g} in {nev[0]} evaluations; scipy {sbound:.9g} in {sev}; difference / 1e-6: {rel / TOL:.3g}")
    assert rel <= TOL


@pytest.mark.parametrize("kid", OPT_JOINT)
def test_joint_optimiser_over_theta_and_z(engine, kid):
    _, th0, _, fixed, _ = run_optimiser(engine, kid, False)
    _, th, Zr, bound, nev = run_optimiser(engine, kid, True)                      # (a) the bitwise re-evaluation, inside
    assert bound[0] >= fixed[0]                                                   # (b) at least the theta-only optimum
    sbound, sev = scipy_run(kid, True)[2:4]
    tight = scipy_run(kid, True, factr=10.0)[2]
    assert scipy_run(kid, True)[5] == 0 and scipy_run(kid, True, factr=10.0)[5] == 0
    gap = abs(tight - sbound)
    slack = max(TOL * max(1.0, abs(sbound)), 10.0 * gap)
    print(f"kernel {kid}: joint bound {bound[0]:.9g} in {nev[0]} evaluations (theta only {fixed[0]:.9g}); scipy {sbound:.9g} in {sev}, "
          f"factr 10 {tight:.9g}: gap {gap:.3g}, device - scipy {bound[0] - sbound:.3g}, allowed -{slack:.3g}")
    assert bound[0] >= sbound - slack                                             # (c)
