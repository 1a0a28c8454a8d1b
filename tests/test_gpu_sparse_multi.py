"""GPU parity and promises of the sparse fits with P target columns (cgp_fit_predict_sparse_multi_batch[_device], include/corenav_gp.h)
through engine.py.  Bars: 1e-6 against tests/sparse_multi_oracle.py in multi_oracle.errors' metric (the project's), bitwise wherever
the header promises it -- which includes promise 4: a column is bitwise the single-column call on that column.  Every problem is
test_gpu_sparse.py's (problem / history) with target columns added on the same inputs -- the same smooth function with a phase and
an amplitude per column, plus noise -- so the oracle's conditions, which depend on (X, Z, theta) alone, are test_gpu_sparse.py's;
test_oracle_sparse_multi.py asserts them on the CPU for the whole list COMPARED.  Against the oracle every column is held to the
one-factor statement and columns 0, P // 2 and P - 1 to the per-column definition.  Shapes sit on the kernels' edges: m + P across
the 16-row tiles and the tile groups of k_sparse_phi, P across the passes of the column solves."""
import numpy as np
import pytest

import sparse_multi_oracle as smo
import test_gpu_sparse as tg

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1
CHUNK = tg.CHUNK
MAX_P = 64           # CGP_SPARSE_MAX_P
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_sparse_multi.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def add_columns(X, theta, kid, P, seed):
    """Y (B, P, N) on the inputs of a test_gpu_sparse problem: one_fit's function with a phase and an amplitude per column."""
    rng = np.random.default_rng(seed + 7919)
    B, N, d = X.shape
    Y = np.empty((B, P, N))
    for b in range(B):
        ell = tg.ells_of(kid, theta[b], d)
        amp = np.sqrt(theta[b, 0] * (theta[b, 2] * 50.0 if kid == 2 else 1.0))
        for p in range(P):
            Y[b, p] = (1.0 + 0.5 * rng.random()) * amp * np.sin(np.sum(X[b] / ell, axis=1) * 0.7 + 0.3 + 2 * np.pi * rng.random()) \
                + np.sqrt(theta[b, -1]) * rng.normal(size=N)
    return Y


def problem(B, N, d, M, m, P, kid, seed):
    X, _, Z, Xs, theta = tg.problem(B, N, d, M, m, kid, seed)
    return X, add_columns(X, theta, kid, P, seed), Z, Xs, theta


def history(N, m, M, P, seed):
    X, y, Z, Xs, theta = tg.history(N, m, M, seed)
    rng = np.random.default_rng(seed + 7919)
    t, ell = X[0, :, 0], theta[0, 1]
    Y = np.stack([0.1 * np.sin(t / ell * 0.9 + 2 * np.pi * rng.random()) + 0.05 * np.cos(t / ell * 0.31 + p)
                  + np.sqrt(1e-3) * rng.normal(size=N) for p in range(P)])
    return X, Y[None], Z, Xs, theta


# every (generator, arguments, fit) compared with the oracle: test_oracle_sparse_multi.py asserts conditions_hold on each
EVERY_KERNEL = tg.EVERY_KERNEL
P_EDGES = [1, 2, 4, 15, 16, 17, 64]
TILE_ROW_EDGES = [(14, 2), (14, 3), (17, 15), (17, 16)]   # m + P = 16 | 17 and 32 | 33: across a 16-row tile of the augmented matrix
GROUP_EDGES = [(270, 2), (270, 3)]                        # m + P = 272: 17 tile rows, 153 tiles, one group; 273: 18, 171, two
# m + P = 576: 36 tile rows, panel stride 16 x 37.  Two sub-panel buffers of 16 samples and the inducing inputs take
# 8 (2 x 16 x 592 + 576 d) bytes: 160 768 <= 160 kB at d = 2 (S = 16), 165 376 > 160 kB at d = 3 (S = 8)
LARGEST = [(512, 64, 2), (512, 64, 3)]
N_EDGES = [1, CHUNK + 1, 2 * CHUNK + 3]
M_EDGES = [0, 1, 16, 65]
HISTORY = (20000, 48, 33, 4, 3)
EXTENT_CASES = [((2, 77, 3, 19, 21, 3), 1), ((3, 531, 1, 5, 33, 18), 2)]   # test_gpu_sparse_multi_extents.py: (B, N, d, M, m, P), kernel
COMPARED = ([("problem", (2, 130, d, 17, 17, 3, kid, 10 * kid + d), b) for kid, d in EVERY_KERNEL for b in (0, 1)]
            + [("problem", (2, 130, 2, 17, 17, P, 1, 500 + P), 1) for P in P_EDGES]
            + [("problem", (2, 130, 2, 17, m, P, 1, 600 + m + P), 1) for m, P in TILE_ROW_EDGES]
            + [("problem", (2, 40, 2, 17, m, P, 1, 700 + P), 1) for m, P in GROUP_EDGES]
            + [("problem", (1, 33, d, 17, m, P, 1, 800 + d), 0) for m, P, d in LARGEST]
            + [("problem", (2, N, 2, 17, 17, 3, 1, 900 + N), 1) for N in N_EDGES]
            + [("problem", (2, 130, 2, M, 17, 3, 1, 1000 + M), 1) for M in M_EDGES]
            + [("history", HISTORY, 0)]
            + [("problem", (3, 200, 2, 30, 40, 5, 1, 9), b) for b in (0, 2)])


def extent_args(shape, kid):
    B, N, d, M, m, P = shape
    return B, N, d, M, m, P, kid, 31 * N + m


COMPARED += [("problem", extent_args(shape, kid), 1) for shape, kid in EXTENT_CASES]


def generate(name, args):
    return {"problem": problem, "history": history}[name](*args)


def oracle_columns(P):
    return sorted({0, P // 2, P - 1})


def ctx_for(engine, B, N, d, M, m, P, max_n=None):
    ctx = tg.ctx_for(engine, B, N, d, M, m, max_n)
    assert ctx.sparse_multi_reserve(B, P) == 0
    return ctx


def close(kid, theta, X, Y, Z, Xs, mean, var, bound, noise=True, tol=TOL, jitter=0.0):
    """One fit against both statements of the oracle; the conditions are asserted on the per-column one."""
    xs = Xs if Xs.shape[0] else None
    o = smo.per_column(kid, theta, X, Y, Z, xs, noise, jitter=jitter, cols=oracle_columns(len(Y)))
    assert o.info == 0 and (jitter > 0.0 or o.ladder == 0) and o.cond_uu <= 1e6 and o.cond_b <= 1e8, (o.info, o.ladder, o.cond_uu, o.cond_b)
    worst = [0.0, 0.0, 0.0]
    for ref in (o, smo.one_factor(kid, theta, X, Y, Z, xs, noise, jitter=o.jitter)):
        worst = [max(a, b) for a, b in zip(worst, smo.errors(mean, var, bound, ref))]
    for k, v in zip(("mean", "var", "bound"), worst):
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    print(f"cond(K_uu) {o.cond_uu:.3g} cond(B) {o.cond_b:.3g}; errors / bar: mean {worst[0] / tol:.3g} var {worst[1] / tol:.3g} "
          f"bound {worst[2] / tol:.3g}")
    assert max(worst) <= tol, worst


def run_and_compare(engine, args, fits, noise=True):
    X, Y, Z, Xs, theta = problem(*args)
    kid = args[6]
    B, N, d = X.shape
    M, m, P = Xs.shape[1], Z.shape[1], Y.shape[1]
    ctx = ctx_for(engine, B, N, d, M, m, P)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs if M else None, theta, kid, include_noise=noise)
    assert rc == 0 and not info.any()
    assert mean.shape == (B, P, M) and var.shape == (B, M) and bound.shape == (B, P)
    for b in fits:
        close(kid, theta[b], X[b], Y[b], Z[b], Xs[b], mean[b], var[b], bound[b], noise)
    return ctx, (X, Y, Z, Xs, theta), (mean, var, bound, info)


def single(ctx, X, y, Z, Xs, theta, kid, noise=True):
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs if Xs.shape[1] else None, theta, kid, include_noise=noise)
    assert rc == 0
    return mean, var, bound, info


def assert_columns_are_the_single_column_call(ctx, arrays, got, kid, cols, noise=True):
    """Promises 2 and 4 on the same context: var and info bitwise, and each column's mean row and bound bitwise."""
    X, Y, Z, Xs, theta = arrays
    mean, var, bound, info = got
    for p in cols:
        m1, v1, b1, i1 = single(ctx, X, Y[:, p], Z, Xs, theta, kid, noise)
        assert np.array_equal(v1, var) and np.array_equal(i1, info), p
        assert np.array_equal(m1, mean[:, p]) and np.array_equal(b1, bound[:, p]), p


@pytest.mark.parametrize("kid,d", EVERY_KERNEL)
def test_every_kernel(engine, kid, d):
    ctx, arrays, got = run_and_compare(engine, (2, 130, d, 17, 17, 3, kid, 10 * kid + d), (0, 1))
    assert_columns_are_the_single_column_call(ctx, arrays, got, kid, range(3))


@pytest.mark.parametrize("P", P_EDGES)
def test_column_count_edges(engine, P):
    ctx, arrays, got = run_and_compare(engine, (2, 130, 2, 17, 17, P, 1, 500 + P), (1,), noise=bool(P % 2))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, oracle_columns(P), noise=bool(P % 2))


@pytest.mark.parametrize("m,P", TILE_ROW_EDGES)
def test_targets_across_a_tile_row(engine, m, P):
    ctx, arrays, got = run_and_compare(engine, (2, 130, 2, 17, m, P, 1, 600 + m + P), (1,))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, (0, P - 1))


@pytest.mark.parametrize("m,P", GROUP_EDGES)
def test_targets_across_a_tile_group(engine, m, P):
    ctx, arrays, got = run_and_compare(engine, (2, 40, 2, 17, m, P, 1, 700 + P), (1,))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, (0, P - 1))


@pytest.mark.parametrize("m,P,d", LARGEST)
def test_largest_augmented_matrix_on_both_sides_of_the_sub_panel_rule(engine, m, P, d):
    """The single-column call at m = 512 runs sub-panels of 16 samples at either d; the multi call 16 at d = 2 and 8 at d = 3: a
    tile element's sum is one chain in sample order whatever the sub-panel is, so the columns stay bitwise."""
    ctx, arrays, got = run_and_compare(engine, (1, 33, d, 17, m, P, 1, 800 + d), (0,))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, (0, P - 1))


@pytest.mark.parametrize("N", N_EDGES)
def test_sample_edges(engine, N):
    assert engine.load().cgp_sparse_chunk() == CHUNK
    ctx, arrays, got = run_and_compare(engine, (2, N, 2, 17, 17, 3, 1, 900 + N), (1,))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, (2,))


@pytest.mark.parametrize("M", M_EDGES)
def test_test_point_edges(engine, M):
    ctx, arrays, got = run_and_compare(engine, (2, 130, 2, M, 17, 3, 1, 1000 + M), (1,), noise=bool(M % 2))
    assert_columns_are_the_single_column_call(ctx, arrays, got, 1, (1,), noise=bool(M % 2))


def test_history_beyond_the_context(engine):
    N, m, M, P, seed = HISTORY
    X, Y, Z, Xs, theta = history(*HISTORY)
    ctx = engine.Context(max_n=128, max_m=64, max_d=1, max_batch=1)
    assert ctx.sparse_reserve(1, N, m, M) == 0 and ctx.sparse_multi_reserve(1, P) == 0
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, 0)
    assert rc == 0 and not info.any()
    close(0, theta[0], X[0], Y[0], Z[0], Xs[0], mean[0], var[0], bound[0])
    assert_columns_are_the_single_column_call(ctx, (X, Y, Z, Xs, theta), (mean, var, bound, info), 0, range(P))


def test_one_column_is_the_single_column_call(engine):
    """P = 1 on the same arrays: (mean, var, logml, info) bitwise -- promise 4's bar as this design keeps it."""
    B, N, d, M, m, kid = 2, 700, 3, 37, 70, 1
    X, Y, Z, Xs, theta = problem(B, N, d, M, m, 1, kid, 10)
    ctx = ctx_for(engine, B, N, d, M, m, 1)
    got = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)
    assert got[0] == 0
    assert_columns_are_the_single_column_call(ctx, (X, Y, Z, Xs, theta), got[1:], kid, (0,))
    close(kid, theta[1], X[1], Y[1], Z[1], Xs[1], got[1][1], got[2][1], got[3][1])


def test_columns_do_not_depend_on_their_number_position_or_neighbours(engine):
    """Promise 3: a permutation of the columns, a prefix of a wide call in a narrow call, and a NaN among one column's targets."""
    B, N, d, M, m, P, kid = 2, 700, 2, 37, 30, 19, 1   # m + P = 49: targets in two tile rows, three passes of the column solves
    X, Y, Z, Xs, theta = problem(B, N, d, M, m, P, kid, 21)
    ctx = ctx_for(engine, B, N, d, M, m, P)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any()
    perm = np.random.default_rng(5).permutation(P)
    rc, pm, pv, pb, pi = ctx.fit_predict_sparse_multi_batch(X, Y[:, perm], Z, Xs, theta, kid)
    assert rc == 0 and np.array_equal(pm, mean[:, perm]) and np.array_equal(pb, bound[:, perm]) and np.array_equal(pv, var)
    for narrow in (1, 3, 8, 9):
        rc, nm, nv, nb, ni = ctx.fit_predict_sparse_multi_batch(X, Y[:, :narrow], Z, Xs, theta, kid)
        assert rc == 0 and np.array_equal(nm, mean[:, :narrow]) and np.array_equal(nb, bound[:, :narrow]) and np.array_equal(nv, var)
    Yn = Y.copy()
    Yn[0, 4, 650] = np.nan   # one sample of one column of fit 0
    rc, qm, qv, qb, qi = ctx.fit_predict_sparse_multi_batch(X, Yn, Z, Xs, theta, kid)
    assert rc == 0 and not qi.any() and np.array_equal(qv, var)
    assert np.all(np.isnan(qm[0, 4])) and np.isnan(qb[0, 4])
    keep = np.ones((B, P), dtype=bool)
    keep[0, 4] = False
    assert np.array_equal(qm[keep], mean[keep]) and np.array_equal(qb[keep], bound[keep])
    close(kid, theta[0], X[0], Y[0], Z[0], Xs[0], mean[0], var[0], bound[0])


def test_slot_batch_and_neighbours_do_not_move_a_fit(engine):
    B, N, d, M, m, P, kid = 3, 200, 2, 30, 40, 5, 1
    X, Y, Z, Xs, theta = problem(B, N, d, M, m, P, kid, 9)
    alone = ctx_for(engine, 1, N, d, M, m, P).fit_predict_sparse_multi_batch(X[:1], Y[:1], Z[:1], Xs[:1], theta[:1], kid)
    assert alone[0] == 0
    ctx = ctx_for(engine, B, N, d, M, m, P)
    for order in ([0, 1, 2], [1, 2, 0]):   # the fit in slot 0 and in slot 2, other neighbours
        Xo, Yo, Zo, Xso, tho = (a[order] for a in (X, Y, Z, Xs, theta))
        rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(Xo, Yo, Zo, Xso, tho, kid)
        assert rc == 0 and not info.any()
        s = order.index(0)
        assert np.array_equal(mean[s], alone[1][0]) and np.array_equal(var[s], alone[2][0]) and np.array_equal(bound[s], alone[3][0])
    close(kid, theta[0], X[0], Y[0], Z[0], Xs[0], alone[1][0], alone[2][0], alone[3][0])


def device_arrays(torch, X, Y, Z, Xs, theta):
    return tg.device_arrays(torch, X, Y, Z, Xs, theta)   # (Y (B, P, N) goes as it is)


def device_outputs(torch, B, P, M, fill=-1.0):
    f = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    return f(B, P, M), f(B, M), f(B, P), torch.full((B,), -1, dtype=torch.int32, device="cuda")


def test_host_device_and_graph_replay_agree_bitwise(engine):
    import torch
    B, N, d, M, m, P, kid = 2, 700, 3, 37, 70, 12, 1   # m + P = 82: targets in two tile rows
    X, Y, Z, Xs, theta = problem(B, N, d, M, m, P, kid, 10)
    ctx = ctx_for(engine, B, N, d, M, m, P)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any()
    dX, dY, dZ, dXs, dth = device_arrays(torch, X, Y, Z, Xs, theta)
    dm, dv, dl, di = device_outputs(torch, B, P, M)

    def clear():
        for t in (dm, dv, dl):
            t.fill_(-1.0)
        di.fill_(-1)
        torch.cuda.synchronize()

    def check():
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dv.cpu().numpy(), var)
        assert np.array_equal(dl.cpu().numpy(), bound) and not di.cpu().numpy().any()

    def enqueue(stream):
        assert ctx.fit_predict_sparse_multi_batch_device(B, N, d, M, P, m, kid, dX.data_ptr(), dY.data_ptr(), dZ.data_ptr(),
                                                         dXs.data_ptr(), dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(),
                                                         dl.data_ptr(), di.data_ptr(), stream) == 0

    clear()
    enqueue(0)
    check()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    clear()
    graph.replay()
    check()


def failing_problem(P=3):
    X, y, Z, Xs, theta, kid = tg.failing_problem()
    return X, add_columns(X, theta, kid, P, 9), Z, Xs, theta, kid   # (targets and noise of fit 1 at its amplitude: theta's own)


def test_failed_fit_is_nan_in_every_column_and_the_neighbours_are_untouched(engine):
    import torch
    X, Y, Z, Xs, theta, kid = failing_problem()
    B, P, N = Y.shape
    d, M, m = X.shape[2], Xs.shape[1], Z.shape[1]
    ctx = ctx_for(engine, B, N, d, M, m, P)
    alone = {b: ctx.fit_predict_sparse_multi_batch(X[b:b + 1], Y[b:b + 1], Z[b:b + 1], Xs[b:b + 1], theta[b:b + 1], kid) for b in (0, 2)}

    def check(mean, var, bound, info):
        assert list(info) == [0, 2, 0]
        assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(bound[1]))
        for b in (0, 2):
            assert np.array_equal(mean[b], alone[b][1][0]) and np.array_equal(var[b], alone[b][2][0]) and np.array_equal(bound[b], alone[b][3][0])

    # device form, no jitter: pivot 2 of K_uu (tg.failing_problem), NaN in all its outputs, neighbours bitwise their stand-alone results
    dX, dY, dZ, dXs, dth = device_arrays(torch, X, Y, Z, Xs, theta)
    dm, dv, dl, di = device_outputs(torch, B, P, M)
    assert ctx.fit_predict_sparse_multi_batch_device(B, N, d, M, P, m, kid, dX.data_ptr(), dY.data_ptr(), dZ.data_ptr(), dXs.data_ptr(),
                                                     dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
    torch.cuda.synchronize()
    check(*(t.cpu().numpy() for t in (dm, dv, dl, di)))
    # host form: a NaN coordinate in the same inducing input is beyond every step of the ladder
    Zn = Z.copy()
    Zn[1, 1, 0] = np.nan
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Zn, Xs, theta, kid)
    assert rc == 2
    check(mean, var, bound, info)


def test_host_form_climbs_the_ladder_with_all_columns(engine):
    """Identical inducing inputs: rescued at the ladder's first step, every column then within 1e-9 of the single-column host call
    (which climbs the same ladder) -- in fact bitwise, the jitter being the same number."""
    X, Y, Z, Xs, theta, kid = failing_problem()
    B, P, N = Y.shape
    ctx = ctx_for(engine, B, N, X.shape[2], Xs.shape[1], Z.shape[1], P)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any()
    for p in range(P):
        m1, v1, b1, i1 = single(ctx, X, Y[:, p], Z, Xs, theta, kid)
        ref = smo.SimpleNamespace(mean=m1[1][None], var=v1[1], bound=b1[1:2], cols=[0])
        e = smo.errors(mean[1, p][None], var[1], bound[1, p:p + 1], ref)
        print(f"column {p}: errors / 1e-9 against the single-column host call: {[v / 1e-9 for v in e]}")
        assert max(e) <= 1e-9 and not i1.any()
    o = smo.per_column(kid, theta[1], X[1], Y[1], Z[1], Xs[1])
    assert o.info == 0 and o.ladder == 1
    e = smo.errors(mean[1], var[1], bound[1], o)
    print(f"ladder step 1, jitter {o.jitter:.3g}; errors / 1e-6: {[v / TOL for v in e]}")
    assert max(e) <= TOL, e


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.zeros(1024)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 40, 1, 4, 2, 3, 2)   # batch, N, d, M, P, m, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, z=p, xs=p, th=p, stride=4, mean=p, var=p):
        return lib.cgp_fit_predict_sparse_multi_batch(h, *shape, x, y, z, xs, th, stride, 1, mean, var, p, ip)

    def dev(h=ctx.h, shape=shape, x=a, y=a, z=a, xs=a, th=a, mean=a, var=a, logml=a, info=a):
        return lib.cgp_fit_predict_sparse_multi_batch_device(h, *shape, x, y, z, xs, th, None, 1, mean, var, logml, info, None)

    bad_counts = ((0, 40, 1, 4, 2, 3, 2), (1, 0, 1, 4, 2, 3, 2), (1, 40, 0, 4, 2, 3, 2), (1, 40, 1, -1, 2, 3, 2), (1, 40, 1, 4, 0, 3, 2),
                  (1, 40, 1, 4, MAX_P + 1, 3, 2), (1, 40, 1, 4, 2, 0, 2), (1, 40, 1, 4, 2, 513, 2), (1, 40, 1, 4, 2, 3, 5), (1, 40, 1, 4, 2, 3, -1))
    assert host() == ESTATE and dev() == ESTATE                                   # no reservation at all
    assert lib.cgp_sparse_multi_reserve(ctx.h, 1, 2) == ESTATE                    # ... and none to size this one by
    for f in (host, dev):                                                         # no context and the counts come first
        assert f(h=None) == EINVAL
        for s in bad_counts:
            assert f(shape=s) == EINVAL, s
    assert lib.cgp_sparse_reserve(ctx.h, 1, 40, 3, 4) == 0
    assert host() == ESTATE and dev() == ESTATE                                   # the sparse reservation alone is not enough
    assert lib.cgp_sparse_multi_reserve(None, 1, 2) == EINVAL
    for mb, mp in ((0, 2), (3, 2), (1, 0), (1, MAX_P + 1)):
        assert lib.cgp_sparse_multi_reserve(ctx.h, mb, mp) == EINVAL
    assert lib.cgp_sparse_multi_reserve(ctx.h, 2, 2) == ESTATE                    # beyond the sparse reservation's batch
    assert lib.cgp_sparse_multi_reserve(ctx.h, 1, 2) == 0
    for s in ((2, 40, 1, 4, 2, 3, 2), (1, 41, 1, 4, 2, 3, 2), (1, 40, 1, 5, 2, 3, 2), (1, 40, 1, 4, 3, 3, 2), (1, 40, 1, 4, 2, 4, 2),
              (1, 40, 2, 4, 2, 3, 1)):
        assert host(shape=s) == ECAPACITY and dev(shape=s) == ECAPACITY, s        # batch, N, M, P, m, d beyond a reservation / the context
        assert host(shape=s, x=None) == ECAPACITY and dev(shape=s, y=None) == ECAPACITY   # ... before the arrays
    for s in bad_counts:                                                          # the counts still come first
        assert host(shape=s) == EINVAL and dev(shape=s) == EINVAL, s
    assert host(shape=(1, 40, 2, 4, 2, 3, 2)) == EINVAL                           # RBF x Brownian needs d = 1
    for k in ("x", "y", "z", "xs", "th", "mean", "var"):
        assert host(**{k: None}) == EINVAL, k
    assert host(stride=3) == EINVAL
    for k in ("x", "y", "z", "xs", "th", "mean", "var", "logml", "info"):
        assert dev(**{k: None}) == EINVAL, k
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_sparse_multi_reserve(f32.h, 1, 2) == EINVAL and host(h=f32.h) == EINVAL and dev(h=f32.h) == EINVAL
    # a later, larger sparse reservation does not widen the multi one; reserving again does
    assert lib.cgp_sparse_reserve(ctx.h, 2, 80, 6, 4) == 0
    assert host(shape=(2, 40, 1, 4, 2, 3, 2)) == ECAPACITY and host(shape=(1, 80, 1, 4, 2, 3, 2)) == ECAPACITY
    assert host(shape=(1, 40, 1, 4, 2, 6, 2)) == ECAPACITY
    assert lib.cgp_sparse_multi_reserve(ctx.h, 2, 2) == 0
    # the context is still usable; M = 0 takes NULL outputs and gives the P bounds only
    X, Y, Z, Xs, theta = problem(2, 80, 1, 4, 6, 2, 2, 2)
    bounds = np.zeros((2, 2))
    assert lib.cgp_fit_predict_sparse_multi_batch(ctx.h, 2, 80, 1, 0, 2, 6, 2, engine._p(X), engine._p(Y), engine._p(Z), None,
                                                  engine._p(theta), 4, 1, None, None, engine._p(bounds), None) == 0
    rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, 2)
    assert rc == 0 and not info.any() and np.array_equal(bound, bounds)
    close(2, theta[0], X[0], Y[0], Z[0], Xs[0], mean[0], var[0], bound[0])
