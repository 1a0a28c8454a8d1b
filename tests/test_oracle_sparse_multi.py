"""tests/sparse_multi_oracle.py is what the GPU tests of the sparse fits with P target columns are held to, so it is pinned here, on
the CPU:
  1. its two statements -- the pinned single-column oracle once per column, and one factorisation with all columns solved at once
     -- agree within 1e-10 on every input the GPU tests compare (columns 0, P // 2 and P - 1 of each: the ones the GPU tests hold to
     the per-column statement);
  2. sum_p logml[p] is GPy's objective of the model: its single-column form with the shared terms taken P times, y^T y replaced by
     tr(Y^T Y) and c^T c by tr(C^T C);
  3. the oracle's conditions (sparse_oracle.conditions_hold: no ladder step, cond(K_uu) <= 1e6, cond(B) <= 1e8 -- functions of (X,
     Z, theta) alone) hold for EVERY input of test_gpu_sparse_multi.py's COMPARED list, and the failure cases' premises;
  4. the engine module exposes the three methods and the header declares the three symbols."""
import os

import numpy as np
import pytest

import sparse_multi_oracle as smo
import sparse_oracle as so
import test_gpu_sparse_multi as tm

from conftest import ROOT

TOL = 1e-10


@pytest.fixture(scope="module")
def compared():
    """Each compared input evaluated once: (kid, arrays of the fit, per-column statement)."""
    out = []
    for name, args, b in tm.COMPARED:
        X, Y, Z, Xs, theta = tm.generate(name, args)
        kid = args[6] if name == "problem" else 0
        xs = Xs[b] if Xs.shape[1] else None
        o = smo.per_column(kid, theta[b], X[b], Y[b], Z[b], xs, cols=tm.oracle_columns(Y.shape[1]))
        out.append(((name, args, b), kid, (theta[b], X[b], Y[b], Z[b], xs), o))
    return out


def test_every_input_the_gpu_tests_compare_meets_the_conditions(compared):
    for tag, kid, arrays, o in compared:
        assert so.conditions_hold(o), (tag, o.info, o.ladder, o.cond_uu, o.cond_b)


def test_the_two_statements_agree(compared):
    worst = 0.0
    for tag, kid, (theta, X, Y, Z, xs), o in compared:
        of = smo.one_factor(kid, theta, X, Y, Z, xs)
        e = smo.errors(of.mean, of.var, of.bound, o)
        worst = max(worst, max(e))
        assert max(e) <= TOL, (tag, e)
    print("largest error / 1e-10 between the two statements:", worst / TOL)


def test_summed_bound_is_gpys_objective_with_the_shared_terms_taken_p_times():
    kid = 1
    X, Y, Z, Xs, theta = tm.problem(1, 130, 2, 0, 17, 5, kid, 77)
    o = smo.per_column(kid, theta[0], X[0], Y[0], Z[0], None)
    of = smo.one_factor(kid, theta[0], X[0], Y[0], Z[0], None)
    P, sigma2 = Y.shape[1], theta[0, -1] + so.DIAG_EPS
    # GPy: P (shared terms) - tr(Y^T Y) / (2 sigma2) + tr(C^T C) / 2
    total = P * of.shared - np.trace(Y[0] @ Y[0].T) / (2.0 * sigma2) + 0.5 * np.trace(of.C.T @ of.C)
    assert abs(np.sum(o.bound) - total) <= TOL * max(1.0, abs(total)), (np.sum(o.bound), total)


def test_premises_of_the_failure_cases():
    X, Y, Z, Xs, theta, kid = tm.failing_problem()
    assert np.array_equal(Z[1, 0], Z[1, 1]) and Y.shape[1] == 3
    no_ladder = smo.per_column(kid, theta[1], X[1], Y[1], Z[1], Xs[1], jitter=1e-300)
    assert no_ladder.info == 2 and np.all(np.isnan(no_ladder.bound)) and np.all(np.isnan(no_ladder.mean))
    climbed = smo.per_column(kid, theta[1], X[1], Y[1], Z[1], Xs[1])
    assert climbed.info == 0 and climbed.ladder == 1 and np.all(np.isfinite(climbed.bound)) and climbed.cond_b <= so.MAX_COND_B
    of = smo.one_factor(kid, theta[1], X[1], Y[1], Z[1], Xs[1], jitter=climbed.jitter)
    assert max(smo.errors(of.mean, of.var, of.bound, climbed)) <= 1e-9
    for b in (0, 2):
        assert so.conditions_hold(smo.per_column(kid, theta[b], X[b], Y[b], Z[b], Xs[b], cols=[0]))


def test_the_engine_exposes_the_calls_and_the_header_declares_them():
    import corenav_gp_amd.engine as engine
    for name in ("sparse_multi_reserve", "fit_predict_sparse_multi_batch", "fit_predict_sparse_multi_batch_device"):
        assert callable(getattr(engine.Context, name, None)), name
    hdr = open(os.path.join(ROOT, "include", "corenav_gp.h")).read()
    for name in ("cgp_sparse_multi_reserve", "cgp_fit_predict_sparse_multi_batch", "cgp_fit_predict_sparse_multi_batch_device"):
        assert f"int {name}(cgp_ctx *ctx" in hdr and name in engine.EXPORTS, name
    assert "#define CGP_SPARSE_MAX_P 64" in hdr
