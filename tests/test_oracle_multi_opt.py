"""CPU checks of the multi-target objective's oracle (tests/multi_opt_oracle.py): the per-column sum against the one-factor
restatement 1/2 (A A^T - P Ky^-1) at 1e-10, and against central differences with test_oracle.py's step and bar."""
import numpy as np
import pytest

import multi_opt_oracle as moo

CASES = [(0, 2), (1, 3), (2, 1), (3, 2), (4, 3)]


def case(kid, d, P=3, N=40):
    rng = np.random.default_rng(11 + kid)
    if kid == 2:
        X = (11.0 + np.arange(N))[:, None]
        theta = np.array([0.7, 12.0, 0.03, 0.02])
    else:
        X = rng.normal(size=(N, d))
        theta = np.concatenate([[0.9], rng.uniform(0.6, 1.8, 1 if kid == 0 else d), [0.08]])
    Y = np.stack([0.2 * np.sin(np.arange(N) / (5.0 + p)) + 0.05 * rng.normal(size=N) for p in range(P)])
    return X, Y, theta


@pytest.mark.parametrize("kid,d", CASES)
def test_column_sum_is_the_one_factor_form(kid, d):
    X, Y, theta = case(kid, d)
    nll, g, lml = moo.nll_and_grad_multi(kid, theta, X, Y)
    nll1, g1 = moo.nll_and_grad_one_factor(kid, theta, X, Y)
    assert lml.shape == (3,) and nll == pytest.approx(-np.sum(lml), rel=1e-14)
    assert abs(nll - nll1) <= 1e-10 * abs(nll)
    assert np.max(np.abs(g - g1)) <= 1e-10 * np.max(np.abs(g))


@pytest.mark.parametrize("kid,d", CASES)
def test_gradient_vs_finite_differences(kid, d):
    X, Y, theta = case(kid, d)
    nll, g, _ = moo.nll_and_grad_multi(kid, theta, X, Y)
    for p in range(len(theta)):
        h = 1e-6 * theta[p]
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        fd = (moo.nll_and_grad_multi(kid, tp, X, Y)[0] - moo.nll_and_grad_multi(kid, tm, X, Y)[0]) / (2 * h)
        assert g[p] == pytest.approx(fd, rel=2e-5, abs=1e-7)


def test_one_column_is_the_single_target_oracle():
    from oracle import gp_oracle as go
    X, Y, theta = case(1, 3, P=1)
    nll, g, _ = moo.nll_and_grad_multi(1, theta, X, Y)
    onll, og = go.nll_and_grad(1, theta, X, Y[0])
    assert nll == onll and np.array_equal(g, og)
