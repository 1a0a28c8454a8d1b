"""GPU parity of the sparse (inducing-point) fits (cgp_fit_predict_sparse_batch[_device]: the collapsed variational bound and its
forecast, include/corenav_gp.h) against tests/sparse_oracle.py, through engine.py.  Bars are the project's: 1e-6 against the oracle in
multi_oracle.errors' metric, bitwise wherever the header promises it.  Every input that is compared with the oracle meets the
oracle's own conditions (sparse_oracle.conditions_hold: no ladder step, cond(K_uu) <= 1e6, cond(B) <= 1e8) -- asserted here, and for
the whole list COMPARED on the CPU by test_oracle_sparse.py, which imports the generators below.  Shapes sit on the edges of the
kernels: m across the 16-row tiles and the tile groups of k_sparse_phi, N across its sub-panels and chunks, M across the 16-column
tiles of k_sparse_predict."""

import numpy as np
import pytest

import sparse_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-6
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1
CHUNK = 512          # cgp_sparse_chunk(): asserted against the library in test_sample_edges
SPACING = 1.25       # inducing inputs, in length-scales: K_uu of a lattice at this spacing has cond ~ 15 per dimension
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_sparse.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def ells_of(kid, theta, d):
    return np.full(d, theta[1]) if kid in (0, 2) else np.asarray(theta[1:1 + d])


def one_fit(N, d, M, m, kid, theta, rng):
    """Inducing inputs: the first m points of a d-dimensional lattice at SPACING length-scales, slightly perturbed; samples and test
    points uniform over the lattice's box; targets a smooth function of the inputs plus noise.  RBF x Brownian: positive inputs."""
    ell = ells_of(kid, theta, d)
    g = int(np.ceil(m ** (1.0 / d) - 1e-9))
    idx = np.array(list(np.ndindex(*([g] * d)))[:m], dtype=np.float64)
    off = 30.0 if kid == 2 else 0.0
    Z = (idx * SPACING + 0.05 * rng.uniform(-1, 1, size=idx.shape)) * ell + off
    hi = idx.max(axis=0) + 0.5 if m > 1 else np.full(d, 0.5)
    box = lambda n: rng.uniform(-0.5, hi, size=(n, d)) * SPACING * ell + off
    X, Xs = box(N), box(M)
    amp = np.sqrt(theta[0] * (theta[2] * 50.0 if kid == 2 else 1.0))
    y = amp * np.sin(np.sum(X / ell, axis=1) * 0.7 + 0.3) + np.sqrt(theta[-1]) * rng.normal(size=N)
    return X, y, Z, Xs


def problem(B, N, d, M, m, kid, seed, theta=None):
    rng = np.random.default_rng(seed)
    th = np.tile(theta_of(kid, d) if theta is None else np.asarray(theta, dtype=np.float64), (B, 1))
    th[:, 0] *= 1.0 + 0.2 * rng.random(B)
    fits = [one_fit(N, d, M, m, kid, th[b], rng) for b in range(B)]
    X, y, Z, Xs = (np.stack([f[i] for f in fits]) for i in range(4))
    return X, y, Z, Xs, th


def history(N, m, M, seed):
    """A long one-dimensional record (tick counts) with m inducing inputs spread over it at SPACING length-scales."""
    rng = np.random.default_rng(seed)
    t = np.arange(N, dtype=np.float64)
    ell = (N - 1) / ((m - 1) * SPACING)
    theta = np.array([[0.02, ell, 1e-3]])
    y = 0.1 * np.sin(t / ell * 0.9) + 0.05 * np.cos(t / ell * 0.31 + 1.0) + np.sqrt(1e-3) * rng.normal(size=N)
    Z = np.linspace(0.0, N - 1.0, m)
    Xs = (N - 1.0) * rng.random(M)
    return t[None, :, None], y[None], Z[None, :, None], Xs[None, :, None], theta


# every (generator, arguments, fit) the tests below compare with the oracle: test_oracle_sparse.py asserts conditions_hold on each
EVERY_KERNEL = [(kid, 3 if kid != 2 else 1) for kid in range(5)]
M_IND_EDGES = [1, 16, 17, 64, 65, 130, 512]
N_EDGES = [1, 3, 63, 65, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
M_EDGES = [0, 1, 16, 65]
HISTORY = (20000, 48, 33, 3)
EXTENT_CASES = [((2, 77, 3, 19, 21), 1), ((3, 531, 1, 5, 33), 2), ((2, 40, 2, 33, 15), 4)]   # test_gpu_sparse_extents.py: (B, N, d, M, m), kernel
COMPARED = ([("problem", (2, 130, d, 17, 17, kid, 10 * kid + d), b) for kid, d in EVERY_KERNEL for b in (0, 1)]
            + [("problem", (2, 130, 2, 17, m, 1, 100 + m), 1) for m in M_IND_EDGES]
            + [("problem", (2, N, 2, 17, 17, 1, 200 + N), 1) for N in N_EDGES]
            + [("problem", (2, 5, 2, 17, 17, 1, 300), 1)]
            + [("problem", (2, 130, 2, M, 17, 1, 400 + M), 1) for M in M_EDGES]
            + [("history", HISTORY, 0)]
            + [("problem", (3, 200, 2, 30, 40, 1, 9), b) for b in (0, 2)])


def extent_args(shape, kid):
    B, N, d, M, m = shape
    return B, N, d, M, m, kid, 31 * N + m


COMPARED += [("problem", extent_args(shape, kid), 1) for shape, kid in EXTENT_CASES]


def generate(name, args):
    return {"problem": problem, "history": history}[name](*args)


def ctx_for(engine, B, N, d, M, m, max_n=None):
    ctx = engine.Context(max_n=max_n or max(16, min(N, 2048)), max_m=max(M, 8), max_d=d, max_batch=B)
    assert ctx.sparse_reserve(B, N, m, M) == 0
    return ctx


def close(kid, theta, X, y, Z, Xs, mean, var, bound, noise=True, tol=TOL, need_conditions=True, jitter=0.0):
    o = so.fit_predict_sparse(kid, theta, X, y, Z, Xs if Xs.shape[0] else None, noise, jitter=jitter)
    if need_conditions:
        assert so.conditions_hold(o), (o.info, o.ladder, o.cond_uu, o.cond_b)
    e = so.errors(mean, var, bound, o)
    for k, v in zip(("mean", "var", "bound"), e):
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    print(f"cond(K_uu) {o.cond_uu:.3g} cond(B) {o.cond_b:.3g}; errors / bar: mean {e[0] / tol:.3g} var {e[1] / tol:.3g} bound {e[2] / tol:.3g}")
    assert max(e) <= tol, e
    return o


def run_and_compare(engine, args, kid, fits, noise=True, max_n=None):
    X, y, Z, Xs, theta = problem(*args)
    B, N, d = X.shape
    M, m = Xs.shape[1], Z.shape[1]
    ctx = ctx_for(engine, B, N, d, M, m, max_n)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs if M else None, theta, kid, include_noise=noise)
    assert rc == 0 and not info.any()
    assert mean.shape == (B, M) and var.shape == (B, M) and bound.shape == (B,)
    for b in fits:
        close(kid, theta[b], X[b], y[b], Z[b], Xs[b], mean[b], var[b], bound[b], noise)


@pytest.mark.parametrize("kid,d", EVERY_KERNEL)
def test_every_kernel(engine, kid, d):
    run_and_compare(engine, (2, 130, d, 17, 17, kid, 10 * kid + d), kid, (0, 1))


@pytest.mark.parametrize("m", M_IND_EDGES)
def test_inducing_edges(engine, m):
    run_and_compare(engine, (2, 130, 2, 17, m, 1, 100 + m), 1, (1,), noise=bool(m % 2))


@pytest.mark.parametrize("N", N_EDGES)
def test_sample_edges(engine, N):
    assert engine.load().cgp_sparse_chunk() == CHUNK
    run_and_compare(engine, (2, N, 2, 17, 17, 1, 200 + N), 1, (1,))


def test_fewer_samples_than_inducing_inputs(engine):
    run_and_compare(engine, (2, 5, 2, 17, 17, 1, 300), 1, (1,))


@pytest.mark.parametrize("M", M_EDGES)
def test_test_point_edges(engine, M):
    run_and_compare(engine, (2, 130, 2, M, 17, 1, 400 + M), 1, (1,), noise=bool(M % 2))


def test_history_beyond_the_context(engine):
    """The feature's reason for existing: N = 20 000 in a context whose dense fits stop at max_n = 128."""
    N, m, M, seed = HISTORY
    X, y, Z, Xs, theta = history(N, m, M, seed)
    ctx = engine.Context(max_n=128, max_m=64, max_d=1, max_batch=1)
    assert ctx.sparse_reserve(1, N, m, M) == 0
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, 0)
    assert rc == 0 and not info.any()
    close(0, theta[0], X[0], y[0], Z[0], Xs[0], mean[0], var[0], bound[0])
    with pytest.raises(engine.CgpError):   # ... and the dense call does stop there
        ctx.fit_predict_batch(X[:, :129], y[:, :129], Xs, theta, 0)


def test_slot_batch_and_neighbours_do_not_move_a_fit(engine):
    B, N, d, M, m, kid = 3, 200, 2, 30, 40, 1
    X, y, Z, Xs, theta = problem(B, N, d, M, m, kid, 9)
    alone = ctx_for(engine, 1, N, d, M, m).fit_predict_sparse_batch(X[:1], y[:1], Z[:1], Xs[:1], theta[:1], kid)
    assert alone[0] == 0
    ctx = ctx_for(engine, B, N, d, M, m)
    pick = lambda order: tuple(a[order] for a in (X, y, Z, Xs, theta))
    for order in ([0, 1, 2], [1, 2, 0]):   # the fit in slot 0 and in slot 2, other neighbours
        Xo, yo, Zo, Xso, tho = pick(order)
        rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(Xo, yo, Zo, Xso, tho, kid)
        assert rc == 0 and not info.any()
        s = order.index(0)
        assert np.array_equal(mean[s], alone[1][0]) and np.array_equal(var[s], alone[2][0]) and bound[s] == alone[3][0]
    close(kid, theta[0], X[0], y[0], Z[0], Xs[0], alone[1][0], alone[2][0], alone[3][0])


def device_arrays(torch, X, y, Z, Xs, theta):
    th = np.zeros((X.shape[0], 10))
    th[:, :theta.shape[1]] = theta
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X.transpose(0, 2, 1), y, Z.transpose(0, 2, 1), Xs.transpose(0, 2, 1), th)]


def device_outputs(torch, B, M, fill=-1.0):
    f = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    return f(B, M), f(B, M), f(B), torch.full((B,), -1, dtype=torch.int32, device="cuda")


def test_host_device_and_graph_replay_agree_bitwise(engine):
    import torch
    B, N, d, M, m, kid = 2, 700, 3, 37, 70, 1
    X, y, Z, Xs, theta = problem(B, N, d, M, m, kid, 10)
    ctx = ctx_for(engine, B, N, d, M, m)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any()
    dX, dy, dZ, dXs, dth = device_arrays(torch, X, y, Z, Xs, theta)
    dm, dv, dl, di = device_outputs(torch, B, M)

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
        assert ctx.fit_predict_sparse_batch_device(B, N, d, M, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dXs.data_ptr(),
                                                   dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(),
                                                   di.data_ptr(), stream) == 0

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


def test_scratch_left_full_of_nan_by_another_shape_does_not_move_a_call(engine):
    B, N, d, M, m, kid = 2, 300, 2, 20, 33, 1
    X, y, Z, Xs, theta = problem(B, N, d, M, m, kid, 12)
    fresh = ctx_for(engine, B, N, d, M, m).fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    ctx = engine.Context(max_n=64, max_m=64, max_d=d, max_batch=B)
    assert ctx.sparse_reserve(B, 1100, 100, 40) == 0
    X2, y2, Z2, Xs2, th2 = problem(B, 1100, d, 40, 100, kid, 13)
    rc, _, _, bound2, info2 = ctx.fit_predict_sparse_batch(X2, np.full_like(y2, np.nan), Z2 * np.nan, Xs2, th2, kid)
    assert rc != 0 and info2.all() and np.all(np.isnan(bound2))   # NaN through every scratch section the next call uses
    again = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    assert again[0] == 0
    for a, f in zip(again[1:], fresh[1:]):
        assert np.array_equal(a, f)


@pytest.mark.parametrize("kid,d", [(1, 2), (2, 1)])
def test_bound_is_below_the_dense_evidence_and_grows_with_an_inducing_input(engine, kid, d):
    """On the device's own numbers: the bound of m inducing inputs <= the bound of m + 1 <= cgp_fit_predict_batch's logml."""
    B, N, M, m = 2, 130, 17, 17
    X, y, Z, Xs, theta = problem(B, N, d, M, m + 1, kid, 50 + kid)
    ctx = ctx_for(engine, B, N, d, M, m + 1)
    rc, _, _, dense, info = ctx.fit_predict_batch(X, y, Xs, theta, kid)
    assert rc == 0 and not info.any()
    rc1, _, _, more, i1 = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    rc0, _, _, less, i0 = ctx.fit_predict_sparse_batch(X, y, Z[:, :m], Xs, theta, kid)
    assert rc0 == 0 and rc1 == 0 and not i0.any() and not i1.any()
    print("dense", dense, "m + 1", more, "m", less)
    assert np.all(more <= dense + 1e-9 * np.abs(dense)) and np.all(less <= more + 1e-9 * np.abs(more))


def failing_problem():
    """Fit 1 of three has two identical inducing inputs under an amplitude of 4^20 ~ 1.1e12 (targets and noise scaled with it).
    The 1e-8 on K_uu's diagonal is below the amplitude's rounding, and a power of four has an exact square root, so the second pivot
    is exactly zero in any IEEE Cholesky: the device form (no ladder) reports pivot 2.  The ladder's jitter is relative -- 1e-6 of
    K_uu's mean diagonal on its first step -- so no amplitude keeps it from making a matrix with a repeated row positive definite
    again: the host form recovers at step 1 (sparse_oracle agrees: test_oracle_sparse.py), and the host failure below needs a NaN."""
    B, N, d, M, m, kid = 3, 200, 2, 30, 40, 1
    X, y, Z, Xs, theta = problem(B, N, d, M, m, kid, 9)
    theta[1, 0] = 4.0 ** 20
    theta[1, -1] = 1e9
    y[1] *= 1e6 / np.sqrt(0.02)
    Z[1, 1] = Z[1, 0]
    return X, y, Z, Xs, theta, kid


def test_failed_fit_is_nan_with_its_pivot_and_the_neighbours_are_untouched(engine):
    import torch
    X, y, Z, Xs, theta, kid = failing_problem()
    B, N, d = X.shape
    M, m = Xs.shape[1], Z.shape[1]
    ctx = ctx_for(engine, B, N, d, M, m)
    alone = {b: ctx.fit_predict_sparse_batch(X[b:b + 1], y[b:b + 1], Z[b:b + 1], Xs[b:b + 1], theta[b:b + 1], kid) for b in (0, 2)}
    # device form, no jitter: pivot 2 of K_uu, NaN outputs, neighbours bitwise their stand-alone results
    dX, dy, dZ, dXs, dth = device_arrays(torch, X, y, Z, Xs, theta)
    dm, dv, dl, di = device_outputs(torch, B, M)
    assert ctx.fit_predict_sparse_batch_device(B, N, d, M, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dXs.data_ptr(),
                                               dth.data_ptr(), 0, True, dm.data_ptr(), dv.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
    torch.cuda.synchronize()
    mean, var, bound, info = (t.cpu().numpy() for t in (dm, dv, dl, di))
    o = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Z[1], Xs[1], jitter=1e-300)   # (a jitter: no ladder in the oracle either)
    assert list(info) == [0, 2, 0] and o.info == 2
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1])) and np.isnan(bound[1])
    for b in (0, 2):
        assert np.array_equal(mean[b], alone[b][1][0]) and np.array_equal(var[b], alone[b][2][0]) and bound[b] == alone[b][3][0]
    # host form: a NaN coordinate in the same inducing input is beyond every step of the ladder
    Zn = Z.copy()
    Zn[1, 1, 0] = np.nan
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Zn, Xs, theta, kid)
    assert rc == 2 and list(info) == [0, 2, 0]
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1])) and np.isnan(bound[1])
    for b in (0, 2):
        assert np.array_equal(mean[b], alone[b][1][0]) and np.array_equal(var[b], alone[b][2][0]) and bound[b] == alone[b][3][0]
        close(kid, theta[b], X[b], y[b], Z[b], Xs[b], mean[b], var[b], bound[b])


def test_host_form_climbs_the_ladder_on_identical_inducing_inputs(engine):
    X, y, Z, Xs, theta, kid = failing_problem()
    B, N, d = X.shape
    M, m = Xs.shape[1], Z.shape[1]
    ctx = ctx_for(engine, B, N, d, M, m)
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any()
    o = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Z[1], Xs[1])
    assert o.info == 0 and o.ladder == 1
    e = so.errors(mean[1], var[1], bound[1], o)
    print(f"ladder step 1, jitter {o.jitter:.3g}, cond(K_uu) {o.cond_uu:.3g}; errors / 1e-6: {[v / TOL for v in e]}")
    assert max(e) <= TOL, e


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.zeros(512)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 40, 1, 4, 3, 2)   # batch, N, d, M, m, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, z=p, xs=p, th=p, stride=4, mean=p, var=p):
        return lib.cgp_fit_predict_sparse_batch(h, *shape, x, y, z, xs, th, stride, 1, mean, var, p, ip)

    def dev(h=ctx.h, shape=shape, x=a, y=a, z=a, xs=a, th=a, mean=a, var=a, logml=a, info=a):
        return lib.cgp_fit_predict_sparse_batch_device(h, *shape, x, y, z, xs, th, None, 1, mean, var, logml, info, None)

    assert host() == ESTATE and dev() == ESTATE                                   # no reservation
    for f in (host, dev):                                                         # no context and the counts come first
        assert f(h=None) == EINVAL
        for s in ((0, 40, 1, 4, 3, 2), (1, 0, 1, 4, 3, 2), (1, 40, 0, 4, 3, 2), (1, 40, 1, -1, 3, 2), (1, 40, 1, 4, 0, 2),
                  (1, 40, 1, 4, 513, 2), (1, 40, 1, 4, 3, 5), (1, 40, 1, 4, 3, -1)):
            assert f(shape=s) == EINVAL, s
    assert lib.cgp_sparse_reserve(None, 1, 40, 3, 4) == EINVAL
    for mb, mn, mi, mm in ((0, 40, 3, 4), (3, 40, 3, 4), (1, 0, 3, 4), (1, 40, 0, 4), (1, 40, 513, 4), (1, 40, 3, -1)):
        assert lib.cgp_sparse_reserve(ctx.h, mb, mn, mi, mm) == EINVAL
    assert host() == ESTATE
    assert lib.cgp_sparse_reserve(ctx.h, 1, 40, 3, 4) == 0                        # N = 40 > the context's max_n = 16: the point
    for s in ((2, 40, 1, 4, 3, 2), (1, 41, 1, 4, 3, 2), (1, 40, 1, 5, 3, 2), (1, 40, 1, 4, 4, 2), (1, 40, 2, 4, 3, 1)):
        assert host(shape=s) == ECAPACITY and dev(shape=s) == ECAPACITY, s        # batch, N, M, m, d beyond the reservation / context
        assert host(shape=s, x=None) == ECAPACITY and dev(shape=s, y=None) == ECAPACITY   # ... before the arrays
    assert host(shape=(1, 40, 2, 4, 3, 2)) == EINVAL                              # RBF x Brownian needs d = 1
    for k in ("x", "y", "z", "xs", "th", "mean", "var"):
        assert host(**{k: None}) == EINVAL, k
    assert host(stride=3) == EINVAL
    for k in ("x", "y", "z", "xs", "th", "mean", "var", "logml", "info"):
        assert dev(**{k: None}) == EINVAL, k
    bound_only = (1, 40, 1, 0, 3, 2)                                              # M = 0: Xs, mean and var may be NULL
    f32 = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2, dtype=F32)
    assert lib.cgp_sparse_reserve(f32.h, 1, 40, 3, 4) == EINVAL and host(h=f32.h) == EINVAL and dev(h=f32.h) == EINVAL
    # the context is still usable, and M = 0 takes NULL outputs
    X, y, Z, Xs, theta = problem(1, 40, 1, 4, 3, 2, 2)
    assert lib.cgp_fit_predict_sparse_batch(ctx.h, *bound_only, engine._p(X), engine._p(y), engine._p(Z), None, engine._p(theta), 4, 1,
                                            None, None, p, ip) == 0
    rc, mean, var, bound, info = ctx.fit_predict_sparse_batch(X, y, Z, Xs, theta, 2)
    assert rc == 0 and not info.any() and bound[0] == buf[0]
    close(2, theta[0], X[0], y[0], Z[0], Xs[0], mean[0], var[0], bound[0])
