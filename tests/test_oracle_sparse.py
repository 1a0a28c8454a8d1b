"""tests/sparse_oracle.py is what the sparse GPU tests are held to, so it is pinned here, on the CPU, three ways:
  1. against the dense N x N statement of the bound and the DTC predictive -- another algebraic route -- evaluated with mpmath at
     50 digits (tests/golden/sparse_mp_k*.npz, written by tests/golden/gen_sparse_golden.py), all five kernels, within 1e-9;
  2. Z = X at eps = 0 is the exact fit of oracle/gp_oracle.py (matern_oracle.py) within 1e-9, on inputs one length-scale apart so
     that K_ff needs no jitter;
  3. the bound is below the exact log marginal likelihood and does not decrease by more than 1e-9 |bound| with one more inducing
     input.
It also asserts the oracle's own conditions (no ladder step, cond(K_uu) <= 1e6, cond(B) <= 1e8) for EVERY input the GPU tests
compare, drawn from test_gpu_sparse.py's own generators, and the premises of its failure cases."""
import glob
import os

import numpy as np
import pytest

from oracle import gp_oracle as go
import matern_oracle as mo
import sparse_oracle as so
import test_gpu_sparse as tg

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-9


def test_golden_fixtures_cover_every_kernel():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "golden", "sparse_mp_k*.npz"))) == \
        [f"sparse_mp_k{k}.npz" for k in range(5)]


@pytest.mark.parametrize("kid", range(5))
def test_oracle_agrees_with_the_dense_statement_at_50_digits(kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_mp_k{kid}.npz"))
    assert int(g["kid"]) == kid and g["X"].shape[0] == 40 and g["Z"].shape[0] == 7
    o = so.fit_predict_sparse(kid, g["theta"], g["X"], g["y"], g["Z"], g["Xs"], noise=False)
    assert so.conditions_hold(o)
    ref = so.SimpleNamespace(mean=g["mean"], var=g["var"], bound=float(g["bound"]))
    e = so.errors(o.mean, o.var, o.bound, ref)
    print("errors / 1e-9:", [v / TOL for v in e])
    assert max(e) <= TOL, e


@pytest.mark.parametrize("kid", range(5))
def test_inducing_inputs_at_the_samples_without_eps_are_the_exact_fit(kid):
    rng = np.random.default_rng(40 + kid)
    N, M, d = 60, 11, 1 if kid == 2 else 2
    theta = tg.theta_of(kid, d)
    ell = tg.ells_of(kid, theta, d)
    g = int(np.ceil(N ** (1.0 / d)))
    idx = np.array(list(np.ndindex(*([g] * d)))[:N], dtype=np.float64)
    X = (idx + 0.1 * rng.uniform(-1, 1, size=idx.shape)) * ell + (30.0 if kid == 2 else 0.0)   # about one length-scale apart
    Xs = rng.uniform(X.min(axis=0), X.max(axis=0), size=(M, d))
    y = np.sqrt(theta[0]) * np.sin(np.sum(X / ell, axis=1)) + np.sqrt(theta[-1]) * rng.normal(size=N)
    ex = mo if kid >= 3 else go
    f = ex.fit(kid, theta, X, y)
    assert f.jitter == 0.0
    mu, var = ex.predict(f, Xs, True)
    o = so.fit_predict_sparse(kid, theta, X, y, X, Xs, noise=True, eps=0.0)
    assert o.info == 0 and o.ladder == 0
    ref = so.SimpleNamespace(mean=mu, var=var, bound=f.logml)
    e = so.errors(o.mean, o.var, o.bound, ref)
    print("errors / 1e-9:", [v / TOL for v in e], "cond(K_uu)", o.cond_uu)
    assert max(e) <= TOL, e


@pytest.mark.parametrize("kid", range(5))
def test_bound_is_below_the_evidence_and_grows_with_an_inducing_input(kid):
    d = 1 if kid == 2 else 3
    X, y, Z, Xs, theta = tg.problem(1, 130, d, 5, 18, kid, 60 + kid)
    exact = (mo if kid >= 3 else go).fit(kid, theta[0], X[0], y[0]).logml
    bounds = [so.fit_predict_sparse(kid, theta[0], X[0], y[0], Z[0, :m], None).bound for m in range(1, 19)]
    print("exact", exact, "bounds", bounds[0], "...", bounds[-1])
    assert all(b <= exact for b in bounds)
    assert all(b1 >= b0 - 1e-9 * abs(b0) for b0, b1 in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("case", range(len(tg.COMPARED)))
def test_every_input_the_gpu_tests_compare_meets_the_conditions(case):
    name, args, b = tg.COMPARED[case]
    X, y, Z, Xs, theta = tg.generate(name, args)
    kid = args[5] if name == "problem" else 0
    o = so.fit_predict_sparse(kid, theta[b], X[b], y[b], Z[b], Xs[b] if Xs.shape[1] else None)
    assert so.conditions_hold(o), (name, args, b, o.info, o.ladder, o.cond_uu, o.cond_b)


def test_premises_of_the_failure_cases():
    X, y, Z, Xs, theta, kid = tg.failing_problem()
    assert np.array_equal(Z[1, 0], Z[1, 1])
    no_ladder = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Z[1], Xs[1], jitter=1e-300)
    assert no_ladder.info == 2 and np.isnan(no_ladder.bound) and np.all(np.isnan(no_ladder.mean))
    # the ladder is relative to K_uu's diagonal: its first step already makes a repeated row positive definite, at any amplitude
    climbed = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Z[1], Xs[1])
    assert climbed.info == 0 and climbed.ladder == 1 and climbed.jitter == so.ladder_jitters(kid, theta[1], Z[1])[0]
    assert np.isfinite(climbed.bound) and climbed.cond_b <= so.MAX_COND_B
    Zn = Z[1].copy()
    Zn[1, 0] = np.nan   # ... a NaN coordinate is beyond every step
    lost = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Zn, Xs[1])
    assert lost.info == 2 and lost.ladder == 5
