"""tests/sparse_grad_oracle.py is what the sparse gradient GPU tests are held to, so it is pinned here, on the CPU:
  1. against the gradient of the dense N x N statement of the bound, differentiated entry by entry with mpmath at 50 digits
     (tests/golden/sparse_grad_mp_k*.npz, written by tests/golden/gen_sparse_grad_golden.py), all five kernels, within 1e-9;
  2. against central differences of tests/sparse_oracle.py's bound -- every component for m <= 64, eight seeded random directions in
     theta and in Z above that -- within 1e-7 of the block's largest component;
  3. for EVERY input the GPU tests compare (test_gpu_sparse_grad.COMPARED): sparse_oracle.conditions_hold and that agreement;
  4. the premises of the optimiser tests: scipy converges, and no trial point of its trajectory needs a ladder step."""
import glob
import os

import numpy as np
import pytest

import sparse_oracle as so
import sparse_grad_oracle as sg
import test_gpu_sparse as tg
import test_gpu_sparse_grad as tgg

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PIN, TOL_FD = 1e-9, 1e-7


def test_golden_fixtures_cover_every_kernel():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "golden", "sparse_grad_mp_k*.npz"))) == \
        [f"sparse_grad_mp_k{k}.npz" for k in range(5)]


@pytest.mark.parametrize("kid", range(5))
def test_oracle_agrees_with_the_dense_gradient_at_50_digits(kid):
    g = np.load(os.path.join(HERE, "golden", f"sparse_grad_mp_k{kid}.npz"))
    f = np.load(os.path.join(HERE, "golden", f"sparse_mp_k{kid}.npz"))
    assert int(g["kid"]) == kid and g["X"].shape[0] == 40 and g["Z"].shape[0] == 7
    for k in ("X", "y", "Z", "theta"):   # gen_sparse_golden.py's problems
        assert np.array_equal(g[k], f[k])
    assert abs(float(g["bound"]) - float(f["bound"])) <= TOL_PIN * max(1.0, abs(float(f["bound"])))
    nll, grad, gz, info = sg.nll_grad(kid, g["theta"], g["X"], g["y"], g["Z"])
    assert info == 0
    e = tgg.errors(nll, grad, gz, -float(g["bound"]), g["grad"], g["gradZ"])
    print("errors / 1e-9:", [v / TOL_PIN for v in e])
    assert max(e) <= TOL_PIN, e


def central_difference_errors(kid, theta, X, y, Z, seed=0):
    """(error of grad, error of gradZ) against central differences of sparse_oracle's bound, each over its block's largest
    component: every component for m <= 64, eight seeded random unit directions per block above that."""
    theta, Z = np.asarray(theta, dtype=np.float64), so._2d(Z)
    m, d = Z.shape
    nth = len(theta)
    nll, g, gz, info = sg.nll_grad(kid, theta, X, y, Z)
    assert info == 0
    f = lambda th, Zz: -so.fit_predict_sparse(kid, th, X, y, Zz, None, jitter=1e-300).bound   # (a jitter: no ladder)
    ell = tg.ells_of(kid, theta, d)
    if m <= 64:
        dirs_t = list(np.eye(nth))
        dirs_z = [e.reshape(m, d) for e in np.eye(m * d)]
    else:
        rng = np.random.default_rng(seed)
        unit = lambda v: v / np.linalg.norm(v)
        dirs_t = [unit(rng.normal(size=nth) * theta) for _ in range(8)]
        dirs_z = [unit(rng.normal(size=(m, d)) * ell) for _ in range(8)]
    # The fourth-order central difference at a step of 1e-4 of the coordinate's scale (theta_i, ell_q): its truncation error is
    # O(1e-16) of the derivative, so what is left is the rounding of the oracle's bound over the step -- at 1e-5 that alone reaches
    # 1e-7 on the longest compared history (the error grows as 1 / h there), at 1e-4 it stays below 4e-8.
    central = lambda fn, h: (-fn(2.0 * h) + 8.0 * fn(h) - 8.0 * fn(-h) + fn(-2.0 * h)) / (12.0 * h)
    et = ez = 0.0
    for u in dirs_t:
        h = 1e-4 * np.min(theta[u != 0] / np.abs(u[u != 0]))
        et = max(et, abs(central(lambda s: f(theta + s * u, Z), h) - g @ u))
    for u in dirs_z:
        h = 1e-4 * np.min((ell * np.ones((m, d)))[u != 0] / np.abs(u[u != 0]))
        ez = max(ez, abs(central(lambda s: f(theta, Z + s * u), h) - np.sum(gz * u)))
    return et / np.max(np.abs(g)), ez / np.max(np.abs(gz))


@pytest.mark.parametrize("case", range(len(tgg.COMPARED)))
def test_every_input_the_gpu_tests_compare_meets_the_conditions_and_central_differences(case):
    name, args, b, kid = tgg.COMPARED[case]
    X, y, Z, theta = tgg.generate(name, args)
    o = so.fit_predict_sparse(kid, theta[b], X[b], y[b], Z[b], None)
    assert so.conditions_hold(o), (name, args, b, o.info, o.ladder, o.cond_uu, o.cond_b)
    et, ez = central_difference_errors(kid, theta[b], X[b], y[b], Z[b], seed=case)
    print(f"cond(K_uu) {o.cond_uu:.3g} cond(B) {o.cond_b:.3g}; central differences / 1e-7: theta {et / TOL_FD:.3g} Z {ez / TOL_FD:.3g}")
    assert et <= TOL_FD and ez <= TOL_FD, (et, ez)


def test_ladder_case_of_the_gpu_tests():
    X, y, Z, Xs, theta, kid = tg.failing_problem()
    nll, g, gz, info, steps, jit = sg.nll_grad_ladder(kid, theta[1], X[1], y[1], Z[1])
    assert info == 0 and steps == 1 and jit == so.ladder_jitters(kid, theta[1], Z[1])[0]
    o = so.fit_predict_sparse(kid, theta[1], X[1], y[1], Z[1], None)
    assert o.ladder == 1 and abs(nll + o.bound) <= 1e-12 * abs(o.bound)
    Zn = Z[1].copy()
    Zn[1, 0] = np.nan
    assert 1 <= sg.nll_grad_ladder(kid, theta[1], X[1], y[1], Zn)[3] <= len(Zn)


@pytest.mark.parametrize("kid", tgg.OPT_THETA)
def test_theta_optimiser_cases_converge_without_a_ladder_step(kid):
    th, Z, bound, evals, warn, ladders = tgg.scipy_run(kid, False)
    X, y, Z0, theta0 = tgg.opt_problem(kid)
    start = so.fit_predict_sparse(kid, theta0[0], X[0], y[0], Z0[0], None).bound
    print(f"kernel {kid}: {start:.6g} -> {bound:.9g} in {evals} evaluations")
    assert warn == 0 and ladders == 0 and bound > start and np.array_equal(Z, Z0[0])
    assert so.conditions_hold(so.fit_predict_sparse(kid, th, X[0], y[0], Z, None))


@pytest.mark.parametrize("kid", tgg.OPT_JOINT)
def test_joint_optimiser_cases_converge_without_a_ladder_step(kid):
    fixed = tgg.scipy_run(kid, False)[2]
    th, Z, bound, evals, warn, ladders = tgg.scipy_run(kid, True)
    tight = tgg.scipy_run(kid, True, factr=10.0)
    print(f"kernel {kid}: joint {bound:.9g} in {evals} evaluations, theta only {fixed:.9g}, factr 10 {tight[2]:.9g} in {tight[3]}")
    # (the factr-10 run may end in the line search, at rounding level: warnflag 2; it only measures the plateau)
    assert warn == 0 and ladders == 0 and tight[4] in (0, 2) and tight[5] == 0 and bound >= fixed and tight[2] >= bound - 1e-3
