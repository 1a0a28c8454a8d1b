"""GPU parity and promises of the sparse fits' objective with P target columns (cgp_sparse_multi_nll_grad_batch[_device],
cgp_optimize_sparse_multi_batch; include/corenav_gp.h) against tests/sparse_multi_grad_oracle.py, through engine.py.  Bars: 1e-6
against the oracle in test_gpu_sparse_grad.errors' metric -- nll against max(1, |nll|), grad and gradZ each against its block's
largest |component| in the oracle --, 1e-9 between two routes of the library (a permutation of the columns; the summed call against
the host sum of P single-column device calls), bitwise wherever the header promises it.  Problems are test_gpu_sparse_multi.py's
(problem / history) without test points; every input that is compared meets sparse_oracle.conditions_hold and agrees with central
differences of the summed bound: asserted for the whole list COMPARED on the CPU by test_oracle_sparse_multi_grad.py.  Shapes sit on
the kernels' edges: P across the passes of the column solves (8 | 9) and the 16-row tiles, m + P across a tile row of the augmented
panel (where the operand image of That leaves A's block) and across a tile group of k_sparse_phi, m across the groups of eight row
tiles of k_sparse_grad_panel, N across its sub-panels and chunks, and the largest panel on both sides of the sub-panel rule."""
import os

import numpy as np
import pytest

import sparse_oracle as so
import sparse_multi_grad_oracle as smg
import test_gpu_sparse as tg
import test_gpu_sparse_grad as tgg
import test_gpu_sparse_multi as tm

pytestmark = pytest.mark.gpu
TOL, TOL_ROUTE = 1e-6, 1e-9
EINVAL, ESTATE, ECAPACITY = -1, -4, -6   # include/corenav_gp.h
F32 = 1
CHUNK = tg.CHUNK
MAX_P = 64
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    yield e
    if WORST:
        print("\nlargest errors / 1e-6 of test_gpu_sparse_multi_grad.py: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in WORST.items()))


def problem(B, N, d, m, P, kid, seed):
    X, Y, Z, _, theta = tm.problem(B, N, d, 0, m, P, kid, seed)
    return X, Y, Z, theta


def history(N, m, P, seed):
    X, Y, Z, _, theta = tm.history(N, m, 0, P, seed)
    return X, Y, Z, theta


def golden(kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_multi_grad_mp_k{kid}.npz"))
    return g["X"][None], g["Y"][None], g["Z"][None], g["theta"][None]


def extent(shape, kid):
    B, N, d, M, m, P = shape
    return problem(B, N, d, m, P, kid, 31 * N + m)


EVERY_KERNEL = tg.EVERY_KERNEL
P_EDGES = [1, 2, 8, 9, 16, 17, 64]                        # 8 | 9: one | two passes of the column solves; 16 | 17: a tile of columns
TILE_ROW_EDGES = [(14, 2), (14, 3), (17, 15), (17, 16)]   # m + P = 16 | 17 and 32 | 33: the image in A's block | in the reservation's
M_IND_EDGES = [127, 128, 129]                             # 128 | 129: one | two groups of row tiles in k_sparse_grad_panel
GROUP_EDGES = [(270, 2), (270, 3)]                        # m + P = 272 | 273: one | two tile groups of k_sparse_phi
LARGEST = [(512, 64, 2), (512, 64, 3)]                    # m + P = 576: sub-panels of 16 samples at d = 2, of 8 at d = 3
N_EDGES = [1, CHUNK + 1, 2 * CHUNK + 3]
HISTORY = (20000, 48, 4, 3)
OPT_THETA = [0, 1, 2, 4]
OPT_JOINT = [1, 4]
# every (generator, arguments, fit, kernel) compared with the oracle: test_oracle_sparse_multi_grad.py asserts the conditions on each
COMPARED = ([("problem", (2, 130, d, 17, 3, kid, 10 * kid + d), b, kid) for kid, d in EVERY_KERNEL for b in (0, 1)]
            + [("golden", (kid,), 0, kid) for kid in range(5)]
            + [("problem", (2, 130, 2, 17, P, 1, 500 + P), 1, 1) for P in P_EDGES]
            + [("problem", (2, 130, 2, m, P, 1, 600 + m + P), 1, 1) for m, P in TILE_ROW_EDGES]
            + [("problem", (2, 130, 2, m, 3, 1, 1100 + m), 1, 1) for m in M_IND_EDGES]
            + [("problem", (2, 40, 2, m, P, 1, 700 + P), 1, 1) for m, P in GROUP_EDGES]
            + [("problem", (1, 33, d, m, P, 1, 800 + d), 0, 1) for m, P, d in LARGEST]
            + [("problem", (2, N, 2, 17, 3, 1, 900 + N), 1, 1) for N in N_EDGES]
            + [("problem", (2, 5, 2, 17, 3, 1, 1200), 1, 1)]
            + [("problem", (2, 130, 1, 33, 3, 2, 1210), 0, 2), ("problem", (2, 700, 3, 70, 5, 3, 1220), 1, 3)]
            + [("history", HISTORY, 0, 0)]
            + [("problem", (3, 200, 2, 40, 5, 1, 9), b, 1) for b in (0, 2)]
            + [("extent", (shape, kid), 1, kid) for shape, kid in tm.EXTENT_CASES]
            + [("problem", (2, 80, 1, 6, 2, 2, 2), 0, 2)])


def generate(name, args):
    return {"problem": problem, "history": history, "golden": golden, "extent": extent}[name](*args)


def opt_problem(kid, P=3):
    return problem(1, 130, 1 if kid == 2 else 3, 17, P, kid, 500 + kid)


def ctx_for(engine, B, N, d, m, P):
    ctx = tgg.ctx_for(engine, B, N, d, m)
    assert ctx.sparse_multi_reserve(B, P) == 0 and ctx.sparse_multi_grad_reserve(B, P) == 0
    return ctx


def column_order_sum(v):
    s = v[0]
    for x in v[1:]:
        s = s + x
    return s


def assert_nll_is_the_column_order_sum(nll, logml):
    for b in range(len(nll)):
        assert nll[b] == -column_order_sum(logml[b]), b


def close(kid, theta, X, Y, Z, nll, g, gz, logml=None, jitter=0.0, need_conditions=True):
    if need_conditions:
        o = so.fit_predict_sparse(kid, theta, X, Y[0], Z, None)
        assert so.conditions_hold(o), (o.info, o.ladder, o.cond_uu, o.cond_b)
    onll, og, ogz, ologml, info = smg.one_factor(kid, theta, X, Y, Z, jitter=jitter)
    assert info == 0
    e = tgg.errors(nll, g, gz, onll, og, ogz)
    names = ["nll", "grad", "gradZ"][:len(e)]
    if logml is not None:
        e.append(float(np.max(np.abs(logml - ologml) / np.maximum(1.0, np.abs(ologml)))))
        names.append("logml")
    for k, v in zip(names, e):
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("errors / bar: " + " ".join(f"{k} {v / TOL:.3g}" for k, v in zip(names, e)))
    assert max(e) <= TOL, e


def run_and_compare(engine, name, args, kid, fits):
    X, Y, Z, theta = generate(name, args)
    B, N, d = X.shape
    m, P = Z.shape[1], Y.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any()
    assert nll.shape == (B,) and g.shape == theta.shape and gz.shape == Z.shape and logml.shape == (B, P)
    assert_nll_is_the_column_order_sum(nll, logml)
    for b in fits:
        close(kid, theta[b], X[b], Y[b], Z[b], nll[b], g[b], gz[b], logml[b])
    return ctx, (X, Y, Z, theta), (nll, g, gz, logml)


def assert_logml_is_the_forward_call(ctx, arrays, logml, kid, M=0):
    """Promise 2: the columns' bounds are bitwise the multi-column forward call's, at M = 0 and at M > 0."""
    X, Y, Z, theta = arrays
    Xs = np.ascontiguousarray(X[:, :M]) if M else None
    rc, _, _, bound, info = ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)
    assert rc == 0 and not info.any() and np.array_equal(bound, logml)


@pytest.mark.parametrize("kid,d", EVERY_KERNEL)
def test_every_kernel(engine, kid, d):
    ctx, arrays, got = run_and_compare(engine, "problem", (2, 130, d, 17, 3, kid, 10 * kid + d), kid, (0, 1))
    assert_logml_is_the_forward_call(ctx, arrays, got[3], kid)


@pytest.mark.parametrize("kid", range(5))
def test_fifty_digit_pins(engine, kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_multi_grad_mp_k{kid}.npz"))
    X, Y, Z, theta = golden(kid)
    ctx = ctx_for(engine, 1, X.shape[1], X.shape[2], Z.shape[1], Y.shape[1])
    rc, nll, gr, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any()
    e = tgg.errors(nll[0], gr[0], gz[0], -float(np.sum(g["bound"])), g["grad"], g["gradZ"])
    e.append(float(np.max(np.abs(logml[0] - g["bound"]) / np.maximum(1.0, np.abs(g["bound"])))))
    print("errors / 1e-6 against the 50-digit dense statement:", [v / TOL for v in e])
    assert max(e) <= TOL, e


@pytest.mark.parametrize("P", P_EDGES)
def test_column_count_edges(engine, P):
    ctx, arrays, got = run_and_compare(engine, "problem", (2, 130, 2, 17, P, 1, 500 + P), 1, (1,))
    assert_logml_is_the_forward_call(ctx, arrays, got[3], 1, M=5)


@pytest.mark.parametrize("m,P", TILE_ROW_EDGES)
def test_targets_across_a_tile_row(engine, m, P):
    run_and_compare(engine, "problem", (2, 130, 2, m, P, 1, 600 + m + P), 1, (1,))


@pytest.mark.parametrize("m", M_IND_EDGES)
def test_inducing_inputs_across_a_group_of_row_tiles(engine, m):
    run_and_compare(engine, "problem", (2, 130, 2, m, 3, 1, 1100 + m), 1, (1,))


@pytest.mark.parametrize("m,P", GROUP_EDGES)
def test_targets_across_a_tile_group_of_phi(engine, m, P):
    run_and_compare(engine, "problem", (2, 40, 2, m, P, 1, 700 + P), 1, (1,))


@pytest.mark.parametrize("m,P,d", LARGEST)
def test_largest_panel_on_both_sides_of_the_sub_panel_rule(engine, m, P, d):
    ctx, arrays, got = run_and_compare(engine, "problem", (1, 33, d, m, P, 1, 800 + d), 1, (0,))
    assert_logml_is_the_forward_call(ctx, arrays, got[3], 1)


@pytest.mark.parametrize("N", N_EDGES)
def test_sample_edges(engine, N):
    assert engine.load().cgp_sparse_chunk() == CHUNK
    run_and_compare(engine, "problem", (2, N, 2, 17, 3, 1, 900 + N), 1, (1,))


def test_fewer_samples_than_inducing_inputs(engine):
    run_and_compare(engine, "problem", (2, 5, 2, 17, 3, 1, 1200), 1, (1,))


def test_other_kernels_across_tiles(engine):
    run_and_compare(engine, "problem", (2, 130, 1, 33, 3, 2, 1210), 2, (0,))
    run_and_compare(engine, "problem", (2, 700, 3, 70, 5, 3, 1220), 3, (1,))


def test_history_beyond_the_context(engine):
    run_and_compare(engine, "history", HISTORY, 0, (0,))


def device_arrays(torch, X, Y, Z, theta):
    return tgg.device_arrays(torch, X, Y, Z, theta)   # (Y (B, P, N) goes as it is)


def device_outputs(torch, B, d, m, P, fill=-1.0):
    f = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda")
    return f(B), f(B, 10), f(B, d, m), f(B, P), torch.full((B,), -1, dtype=torch.int32, device="cuda")


def single_device(torch, ctx, B, N, d, m, kid, dX, dy, dZ, dth):
    dn, dg, dgz, _, di = device_outputs(torch, B, d, m, 1)
    assert ctx.sparse_nll_grad_batch_device(B, N, d, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0,
                                            dn.data_ptr(), dg.data_ptr(), 10, dgz.data_ptr(), di.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not di.cpu().numpy().any()
    return dn.cpu().numpy(), dg.cpu().numpy(), dgz.cpu().numpy().transpose(0, 2, 1)


def test_one_column_is_the_single_column_call_and_the_sum_of_single_column_calls(engine):
    """Promise 3: P = 1 is bitwise the single-column call, host and device.  And the summed call against the host sum of P
    single-column device calls, within 1e-9; the single-column call after it is bitwise what it was (promise 7)."""
    import torch
    B, N, d, m, P, kid = 2, 700, 3, 70, 5, 1
    X, Y, Z, theta = problem(B, N, d, m, P, kid, 10)
    nth = theta.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    before = ctx.sparse_nll_grad_batch(X, Y[:, 2], Z, theta, kid)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any() and before[0] == 0
    after = ctx.sparse_nll_grad_batch(X, Y[:, 2], Z, theta, kid)
    for a, b in zip(before[1:], after[1:]):
        assert np.array_equal(a, b)
    rc, n1, g1, gz1, l1, i1 = ctx.sparse_multi_nll_grad_batch(X, Y[:, 2:3], Z, theta, kid)
    assert rc == 0 and np.array_equal(n1, before[1]) and np.array_equal(g1, before[2]) and np.array_equal(gz1, before[3])
    assert np.array_equal(l1[:, 0], logml[:, 2]) and np.array_equal(-l1[:, 0], n1)
    sn, sgr, sgz = np.zeros(B), np.zeros((B, nth)), np.zeros((B, m, d))
    for p in range(P):
        dX, dy, dZ, dth = tgg.device_arrays(torch, X, Y[:, p], Z, theta)
        n, gr, gzp = single_device(torch, ctx, B, N, d, m, kid, dX, dy, dZ, dth)
        if p == 2:   # the device form of the single-column call, and of this call at P = 1
            assert np.array_equal(n, before[1]) and np.array_equal(gr[:, :nth], before[2]) and np.array_equal(gzp, before[3])
            dn, dg, dgz, dl, di = device_outputs(torch, B, d, m, 1)
            assert ctx.sparse_multi_nll_grad_batch_device(B, N, d, 1, m, kid, dX.data_ptr(), dy.data_ptr(), dZ.data_ptr(), dth.data_ptr(),
                                                          0, dn.data_ptr(), dg.data_ptr(), 10, dgz.data_ptr(), dl.data_ptr(),
                                                          di.data_ptr()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(dn.cpu().numpy(), n) and np.array_equal(dg.cpu().numpy(), gr)
            assert np.array_equal(dgz.cpu().numpy().transpose(0, 2, 1), gzp)
        sn, sgr, sgz = sn + n, sgr + gr[:, :nth], sgz + gzp
    for b in range(B):
        e = tgg.errors(nll[b], g[b], gz[b], sn[b], sgr[b], sgz[b])
        print(f"fit {b}: errors / 1e-9 against the sum of {P} single-column device calls: {[v / TOL_ROUTE for v in e]}")
        assert max(e) <= TOL_ROUTE, e
    close(kid, theta[1], X[1], Y[1], Z[1], nll[1], g[1], gz[1], logml[1])


def test_a_permutation_of_the_columns_and_a_nan_column(engine):
    """Promise 8: a permutation permutes logml bitwise and moves nll, grad and gradZ by no more than 1e-9.  Promise 9: a NaN among
    one column's targets."""
    B, N, d, m, P, kid = 2, 700, 2, 30, 19, 1   # m + P = 49: targets in two tile rows, three passes of the column solves
    X, Y, Z, theta = problem(B, N, d, m, P, kid, 21)
    ctx = ctx_for(engine, B, N, d, m, P)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any()
    perm = np.random.default_rng(5).permutation(P)
    rc, pn, pg, pgz, pl, pi = ctx.sparse_multi_nll_grad_batch(X, Y[:, perm], Z, theta, kid)
    assert rc == 0 and not pi.any() and np.array_equal(pl, logml[:, perm])
    for b in range(B):
        e = tgg.errors(pn[b], pg[b], pgz[b], nll[b], g[b], gz[b])
        print(f"fit {b}: errors / 1e-9 under a permutation of the columns: {[v / TOL_ROUTE for v in e]}")
        assert max(e) <= TOL_ROUTE, e
    Yn = Y.copy()
    Yn[0, 4, 650] = np.nan   # one sample of one column of fit 0
    rc, qn, qg, qgz, ql, qi = ctx.sparse_multi_nll_grad_batch(X, Yn, Z, theta, kid)
    assert rc == 0 and not qi.any()
    assert np.isnan(qn[0]) and np.all(np.isnan(qg[0])) and np.all(np.isnan(qgz[0])) and np.isnan(ql[0, 4])
    keep = np.ones((B, P), dtype=bool)
    keep[0, 4] = False
    assert np.array_equal(ql[keep], logml[keep])
    assert qn[1] == nll[1] and np.array_equal(qg[1], g[1]) and np.array_equal(qgz[1], gz[1])
    close(kid, theta[0], X[0], Y[0], Z[0], nll[0], g[0], gz[0], logml[0])


def test_slot_batch_and_neighbours_do_not_move_a_fit(engine):
    B, N, d, m, P, kid = 3, 200, 2, 40, 5, 1
    X, Y, Z, theta = problem(B, N, d, m, P, kid, 9)
    alone = ctx_for(engine, 1, N, d, m, P).sparse_multi_nll_grad_batch(X[:1], Y[:1], Z[:1], theta[:1], kid)
    assert alone[0] == 0
    ctx = ctx_for(engine, B, N, d, m, P)
    for order in ([0, 1, 2], [1, 2, 0]):
        rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X[order], Y[order], Z[order], theta[order], kid)
        assert rc == 0 and not info.any()
        s = order.index(0)
        assert nll[s] == alone[1][0] and np.array_equal(g[s], alone[2][0]) and np.array_equal(gz[s], alone[3][0])
        assert np.array_equal(logml[s], alone[4][0])
    close(kid, theta[0], X[0], Y[0], Z[0], alone[1][0], alone[2][0], alone[3][0], alone[4][0])


def test_host_device_and_graph_replay_agree_bitwise_with_and_without_the_optional_outputs(engine):
    import torch
    B, N, d, m, P, kid = 2, 700, 3, 70, 12, 1   # m + P = 82: targets in two tile rows
    X, Y, Z, theta = problem(B, N, d, m, P, kid, 10)
    nth = theta.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any()
    assert_nll_is_the_column_order_sum(nll, logml)
    assert_logml_is_the_forward_call(ctx, (X, Y, Z, theta), logml, kid, M=8)
    # promise 6 in the host form
    rc, n0, g0, none, l0, i0 = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid, want_grad_z=False)
    assert rc == 0 and none is None and np.array_equal(n0, nll) and np.array_equal(g0, g) and np.array_equal(l0, logml)
    rc, n0, g0, gz0, none, i0 = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid, want_logml=False)
    assert rc == 0 and none is None and np.array_equal(n0, nll) and np.array_equal(g0, g) and np.array_equal(gz0, gz)
    dX, dY, dZ, dth = device_arrays(torch, X, Y, Z, theta)
    dn, dg, dgz, dl, di = device_outputs(torch, B, d, m, P)

    def clear():
        for t in (dn, dg, dgz, dl):
            t.fill_(-1.0)
        di.fill_(-1)
        torch.cuda.synchronize()

    def check(with_z=True, with_l=True):
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(dn.cpu().numpy(), nll) and np.array_equal(dg.cpu().numpy()[:, :nth], g)
        assert np.all(dg.cpu().numpy()[:, nth:] == -1.0) and not di.cpu().numpy().any()
        assert np.array_equal(dgz.cpu().numpy().transpose(0, 2, 1), gz) if with_z else np.all(dgz.cpu().numpy() == -1.0)
        assert np.array_equal(dl.cpu().numpy(), logml) if with_l else np.all(dl.cpu().numpy() == -1.0)

    def enqueue(stream, with_z=True, with_l=True):
        assert ctx.sparse_multi_nll_grad_batch_device(B, N, d, P, m, kid, dX.data_ptr(), dY.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0,
                                                      dn.data_ptr(), dg.data_ptr(), 10, dgz.data_ptr() if with_z else 0,
                                                      dl.data_ptr() if with_l else 0, di.data_ptr(), stream) == 0

    for with_z, with_l in ((True, True), (False, True), (True, False)):
        clear()
        enqueue(0, with_z, with_l)
        check(with_z, with_l)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    clear()
    graph.replay()
    check()
    # promise 7: the forward calls after this call are what a context that never ran it returns
    Xs = np.ascontiguousarray(X[:, :19])
    fresh = tm.ctx_for(engine, B, N, d, 19, m, P)
    assert ctx.sparse_reserve(B, N, m, 19) == 0 and ctx.sparse_grad_reserve(B) == 0 and ctx.sparse_multi_reserve(B, P) == 0
    assert ctx.sparse_multi_grad_reserve(B, P) == 0
    assert ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)[0] == 0
    for a, b in zip(fresh.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid), ctx.fit_predict_sparse_multi_batch(X, Y, Z, Xs, theta, kid)):
        assert np.array_equal(a, b)
    assert ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)[0] == 0
    for a, b in zip(fresh.fit_predict_sparse_batch(X, Y[:, 1], Z, Xs, theta, kid), ctx.fit_predict_sparse_batch(X, Y[:, 1], Z, Xs, theta, kid)):
        assert np.array_equal(a, b)


def test_scratch_left_full_of_nan_by_another_shape_does_not_move_a_call(engine):
    B, N, d, m, P, kid = 2, 300, 2, 33, 4, 1
    X, Y, Z, theta = problem(B, N, d, m, P, kid, 12)
    fresh = ctx_for(engine, B, N, d, m, P).sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    ctx = ctx_for(engine, B, 1100, d, 100, 20)
    X2, Y2, Z2, th2 = problem(B, 1100, d, 100, 20, kid, 13)
    Y2[:] = np.nan   # K_uu and B factor, and NaN runs through every scratch section the next call uses
    rc, nll2, g2, gz2, l2, info2 = ctx.sparse_multi_nll_grad_batch(X2, Y2, Z2, th2, kid)
    assert np.all(np.isnan(nll2)) and np.all(np.isnan(g2)) and np.all(np.isnan(gz2)) and np.all(np.isnan(l2)) and not info2.any()
    again = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert again[0] == 0 and fresh[0] == 0
    for a, f in zip(again[1:], fresh[1:]):
        assert np.array_equal(a, f)
    single = ctx.sparse_nll_grad_batch(X, Y[:, 1], Z, theta, kid)
    ref = tgg.ctx_for(engine, B, N, d, m).sparse_nll_grad_batch(X, Y[:, 1], Z, theta, kid)
    for a, f in zip(single[1:], ref[1:]):
        assert np.array_equal(a, f)


def test_failed_fit_is_nan_with_its_pivot_and_the_neighbours_are_untouched(engine):
    import torch
    X, Y, Z, _, theta, kid = tm.failing_problem()
    B, P, N = Y.shape
    d, m = X.shape[2], Z.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    alone = {b: ctx.sparse_multi_nll_grad_batch(X[b:b + 1], Y[b:b + 1], Z[b:b + 1], theta[b:b + 1], kid) for b in (0, 2)}
    # device form, no jitter: pivot 2 of K_uu (tg.failing_problem: two identical inducing inputs)
    dX, dY, dZ, dth = device_arrays(torch, X, Y, Z, theta)
    dn, dg, dgz, dl, di = device_outputs(torch, B, d, m, P)
    assert ctx.sparse_multi_nll_grad_batch_device(B, N, d, P, m, kid, dX.data_ptr(), dY.data_ptr(), dZ.data_ptr(), dth.data_ptr(), 0,
                                                  dn.data_ptr(), dg.data_ptr(), 10, dgz.data_ptr(), dl.data_ptr(), di.data_ptr()) == 0
    torch.cuda.synchronize()
    nth = theta.shape[1]
    nll, g, gz, logml, info = (dn.cpu().numpy(), dg.cpu().numpy()[:, :nth], dgz.cpu().numpy().transpose(0, 2, 1), dl.cpu().numpy(),
                               di.cpu().numpy())
    assert list(info) == [0, 2, 0]
    assert np.isnan(nll[1]) and np.all(np.isnan(g[1])) and np.all(np.isnan(gz[1])) and np.all(np.isnan(logml[1]))
    for b in (0, 2):
        assert nll[b] == alone[b][1][0] and np.array_equal(g[b], alone[b][2][0]) and np.array_equal(gz[b], alone[b][3][0])
        assert np.array_equal(logml[b], alone[b][4][0])
    # host form: a NaN coordinate is beyond every step of the ladder
    Zn = Z.copy()
    Zn[1, 1, 0] = np.nan
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Zn, theta, kid)
    assert 1 <= rc <= m and list(info) == [0, rc, 0]
    assert np.isnan(nll[1]) and np.all(np.isnan(g[1])) and np.all(np.isnan(gz[1])) and np.all(np.isnan(logml[1]))
    for b in (0, 2):
        assert nll[b] == alone[b][1][0] and np.array_equal(g[b], alone[b][2][0]) and np.array_equal(gz[b], alone[b][3][0])


def test_host_form_climbs_the_ladder_with_all_columns(engine):
    X, Y, Z, _, theta, kid = tm.failing_problem()
    B, P, N = Y.shape
    ctx = ctx_for(engine, B, N, X.shape[2], Z.shape[1], P)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    assert rc == 0 and not info.any()
    onll, og, ogz, ologml, oinfo, steps, jit = smg.nll_grad_ladder(kid, theta[1], X[1], Y[1], Z[1])
    assert oinfo == 0 and steps == 1
    e = tgg.errors(nll[1], g[1], gz[1], onll, og, ogz)
    print(f"ladder step 1, jitter {jit:.3g}; errors / 1e-6: {[v / TOL for v in e]}")
    assert max(e) <= TOL, e


def test_argument_and_state_errors(engine):
    ctx = engine.Context(max_n=16, max_m=8, max_d=1, max_batch=2)
    buf = np.ones(1024)
    ib = np.zeros(4, dtype=np.int32)
    p, a, ip = engine._p(buf), buf.ctypes.data, ib.ctypes.data_as(engine._ip)
    lib = ctx.lib
    shape = (1, 40, 1, 2, 3, 2)   # batch, N, d, P, m, kernel

    def host(h=ctx.h, shape=shape, x=p, y=p, z=p, th=p, stride=4, nll=p, grad=p, gstride=4, gz=p, lm=p):
        return lib.cgp_sparse_multi_nll_grad_batch(h, *shape, x, y, z, th, stride, nll, grad, gstride, gz, lm, ip)

    def dev(h=ctx.h, shape=shape, x=a, y=a, z=a, th=a, nll=a, grad=a, gstride=4, gz=a, lm=a, info=a):
        return lib.cgp_sparse_multi_nll_grad_batch_device(h, *shape, x, y, z, th, None, nll, grad, gstride, gz, lm, info, None)

    def opt(h=ctx.h, shape=shape, x=p, y=p, z=p, th=p, stride=4):
        return lib.cgp_optimize_sparse_multi_batch(h, *shape, x, y, z, th, stride, 1, 5, None, None)

    calls = (host, dev, opt)
    bad_counts = ((0, 40, 1, 2, 3, 2), (1, 0, 1, 2, 3, 2), (1, 40, 0, 2, 3, 2), (1, 40, 1, 0, 3, 2), (1, 40, 1, MAX_P + 1, 3, 2),
                  (1, 40, 1, 2, 0, 2), (1, 40, 1, 2, 513, 2), (1, 40, 1, 2, 3, 5), (1, 40, 1, 2, 3, -1))
    reserves = (lambda: lib.cgp_sparse_reserve(ctx.h, 1, 40, 3, 4), lambda: lib.cgp_sparse_grad_reserve(ctx.h, 1),
                lambda: lib.cgp_sparse_multi_reserve(ctx.h, 1, 2))
    for f in calls:                                                               # no context and the counts come first
        assert f(h=None) == EINVAL
        for s in bad_counts:
            assert f(shape=s) == EINVAL, s
    for reserve in reserves:                                                      # each missing reservation, in turn
        assert all(f() == ESTATE for f in calls)
        assert lib.cgp_sparse_multi_grad_reserve(ctx.h, 1, 2) == ESTATE           # ... nor can there be one of this section's
        assert reserve() == 0
    assert all(f() == ESTATE for f in calls)                                      # the three others alone are not enough
    assert lib.cgp_sparse_multi_grad_reserve(None, 1, 2) == EINVAL
    for mb, mp in ((0, 2), (3, 2), (1, 0), (1, MAX_P + 1)):
        assert lib.cgp_sparse_multi_grad_reserve(ctx.h, mb, mp) == EINVAL
    assert lib.cgp_sparse_multi_grad_reserve(ctx.h, 2, 2) == ESTATE               # beyond the other reservations' batch
    assert lib.cgp_sparse_multi_grad_reserve(ctx.h, 1, 3) == ESTATE               # ... and the multi reservation's columns
    assert lib.cgp_sparse_multi_grad_reserve(ctx.h, 1, 2) == 0
    for f in calls:
        for s in ((2, 40, 1, 2, 3, 2), (1, 41, 1, 2, 3, 2), (1, 40, 1, 3, 3, 2), (1, 40, 1, 2, 4, 2), (1, 40, 2, 2, 3, 1)):
            assert f(shape=s) == ECAPACITY, s                                     # batch, N, P, m, d beyond the reservations / context
            assert f(shape=s, x=None) == ECAPACITY                                # ... before the arrays
        for s in bad_counts:                                                      # the counts still come first
            assert f(shape=s) == EINVAL, s
        assert f(shape=(1, 40, 2, 2, 3, 2)) == EINVAL                             # RBF x Brownian needs d = 1
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
    assert lib.cgp_sparse_multi_grad_reserve(f32.h, 1, 2) == EINVAL and all(f(h=f32.h) == EINVAL for f in calls)
    # a later, larger reservation of the others does not widen this one; reserving again does
    assert lib.cgp_sparse_reserve(ctx.h, 2, 80, 6, 4) == 0 and lib.cgp_sparse_grad_reserve(ctx.h, 2) == 0
    assert lib.cgp_sparse_multi_reserve(ctx.h, 2, 2) == 0
    assert host(shape=(2, 40, 1, 2, 3, 2)) == ECAPACITY and host(shape=(1, 40, 1, 2, 6, 2)) == ECAPACITY
    assert lib.cgp_sparse_multi_grad_reserve(ctx.h, 2, 2) == 0
    # the context is still usable; gradZ, logml and info may be NULL in the host form
    X, Y, Z, theta = problem(2, 80, 1, 6, 2, 2, 2)
    out_n, out_g = np.zeros(2), np.zeros((2, 4))
    assert lib.cgp_sparse_multi_nll_grad_batch(ctx.h, 2, 80, 1, 2, 6, 2, engine._p(X), engine._p(Y), engine._p(Z), engine._p(theta), 4,
                                               engine._p(out_n), engine._p(out_g), 4, None, None, None) == 0
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, 2)
    assert rc == 0 and np.array_equal(nll, out_n) and np.array_equal(g, out_g)
    close(2, theta[0], X[0], Y[0], Z[0], nll[0], g[0], gz[0], logml[0])


def test_symbols_exported(engine):
    for name in ("cgp_sparse_multi_grad_reserve", "cgp_sparse_multi_nll_grad_batch", "cgp_sparse_multi_nll_grad_batch_device",
                 "cgp_optimize_sparse_multi_batch"):
        assert name in engine.EXPORTS and hasattr(engine.load(), name)


# ---- optimiser ---------------------------------------------------------------------------------------------------
_SCIPY = {}


def scipy_run(kid, optimize_z, factr=1e7):
    """scipy on the oracle from the optimiser tests' start, computed once per (kernel, mode, factr)."""
    key = (kid, optimize_z, factr)
    if key not in _SCIPY:
        X, Y, Z, theta = opt_problem(kid)
        _SCIPY[key] = smg.optimize_sparse_multi(kid, X[0], Y[0], Z[0], theta[0], optimize_z, factr=factr)
    return _SCIPY[key]


def run_optimiser(engine, kid, optimize_z):
    X, Y, Z, theta = opt_problem(kid)
    B, N, d = X.shape
    m, P = Z.shape[1], Y.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    th, Zr, bound, nev = ctx.optimize_sparse_multi_batch(X, Y, Z, theta, kid, optimize_z=optimize_z)
    assert np.all(th > 0) and (optimize_z or np.array_equal(Zr, Z))
    # the column-order sum of the bounds a fresh forward call returns at the returned point, bitwise
    rc, _, _, again, info = ctx.fit_predict_sparse_multi_batch(X, Y, Zr, None, th, kid)
    assert rc == 0 and not info.any() and bound[0] == column_order_sum(again[0])
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
    assert scipy_run(kid, True)[4] == 0 and scipy_run(kid, True)[5] == 0 and scipy_run(kid, True, factr=10.0)[5] == 0
    gap = abs(tight - sbound)
    slack = max(TOL * max(1.0, abs(sbound)), 10.0 * gap)
    print(f"kernel {kid}: joint bound {bound[0]:.9g} in {nev[0]} evaluations (theta only {fixed[0]:.9g}); scipy {sbound:.9g} in {sev}, "
          f"factr 10 {tight:.9g}: gap {gap:.3g}, device - scipy {bound[0] - sbound:.3g}, allowed -{slack:.3g}")
    assert bound[0] >= sbound - slack                                             # (c)


def test_identical_columns_are_p_times_the_single_column_objective(engine):
    kid, P = 1, 3
    X, Y, Z, theta = opt_problem(kid)
    Y = np.ascontiguousarray(np.repeat(Y[:, :1], P, axis=1))
    B, N, d = X.shape
    m = Z.shape[1]
    ctx = ctx_for(engine, B, N, d, m, P)
    rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(X, Y, Z, theta, kid)
    rc1, n1, g1, gz1, i1 = ctx.sparse_nll_grad_batch(X, Y[:, 0], Z, theta, kid)
    assert rc == 0 and rc1 == 0
    e = tgg.errors(nll[0], g[0], gz[0], P * n1[0], P * g1[0], P * gz1[0])
    print(f"errors / 1e-9 against {P} times the single-column call: {[v / TOL_ROUTE for v in e]}")
    assert max(e) <= TOL_ROUTE, e
    th, Zr, bound, nev = ctx.optimize_sparse_multi_batch(X, Y, Z, theta, kid, optimize_z=False)
    th1, Z1, b1, nev1 = ctx.optimize_sparse_batch(X, Y[:, 0], Z, theta, kid, optimize_z=False)
    rel = np.max(np.abs(th - th1) / th1)
    print(f"theta {th[0]} against the single-column optimum {th1[0]}: difference / 1e-6 {rel / TOL:.3g}; bound {bound[0]:.9g} = {P} x {b1[0]:.9g}")
    assert rel <= TOL
