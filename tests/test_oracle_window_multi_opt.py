"""CPU checks of the multi-target windows' objective oracle (tests/window_multi_opt_oracle.py): against the one-factor
restatement 1/2 (A A^T - P Ky^-1) at 1e-10, against central differences with test_oracle_multi_opt.py's step and bar, against the
sum over the columns of tests/adapt_oracle.py::window_nll_grad, and the empty-window rule.  Also asserted here, without a GPU: no
window that tests/test_gpu_window_multi_opt.py compares needs jitter in the oracle's refit -- the resident windows have no ladder,
so the GPU test may skip nothing."""
import numpy as np
import pytest

import adapt_oracle as ao
import multi_opt_oracle as moo
import window_multi_opt_oracle as wmo
import window_multi_oracle as wm

CASES = [(0, 33, 2, 3, 20), (1, 24, 3, 5, 61), (2, 16, 1, 4, 40), (3, 40, 2, 3, 57), (4, 32, 3, 2, 32)]   # kid, N, d, P, T


@pytest.mark.parametrize("kid,N,d,P,T", CASES)
def test_window_objective_is_the_one_factor_form_on_the_last_samples(kid, N, d, P, T):
    X, Y = wm.stream(T, d, P, 7)
    theta = wm.theta_of(kid, d)
    nll, g, lml = wmo.nll_and_grad_multi(kid, theta, N, X, Y)
    n = min(T, N)
    nll1, g1 = moo.nll_and_grad_one_factor(kid, theta, X[-n:], Y[-n:].T)
    assert lml.shape == (P,) and nll == pytest.approx(-np.sum(lml), rel=1e-14)
    assert abs(nll - nll1) <= 1e-10 * abs(nll)
    assert np.max(np.abs(g - g1)) <= 1e-10 * np.max(np.abs(g))
    # a tick count in the middle of the stream
    t = T - 5
    nll2, g2, _ = wmo.nll_and_grad_multi(kid, theta, N, X, Y, t)
    nll3, g3 = moo.nll_and_grad_one_factor(kid, theta, X[max(0, t - N):t], Y[max(0, t - N):t].T)
    assert abs(nll2 - nll3) <= 1e-10 * abs(nll2) and np.max(np.abs(g2 - g3)) <= 1e-10 * np.max(np.abs(g2))


@pytest.mark.parametrize("kid,N,d,P,T", CASES)
def test_gradient_vs_finite_differences(kid, N, d, P, T):
    X, Y = wm.stream(T, d, P, 7)
    theta = wm.theta_of(kid, d)
    _, g, _ = wmo.nll_and_grad_multi(kid, theta, N, X, Y)
    for p in range(len(theta)):
        h = 1e-6 * theta[p]
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        fd = (wmo.nll_and_grad_multi(kid, tp, N, X, Y)[0] - wmo.nll_and_grad_multi(kid, tm, N, X, Y)[0]) / (2 * h)
        assert g[p] == pytest.approx(fd, rel=2e-5, abs=1e-7)


@pytest.mark.parametrize("kid,N,d,P,T", [c for c in CASES if c[0] < 3])
def test_objective_is_the_sum_of_the_single_target_window_oracle(kid, N, d, P, T):
    X, Y = wm.stream(T, d, P, 7)
    theta = wm.theta_of(kid, d)
    for t in (3, T):
        nll, g, lml = wmo.nll_and_grad_multi(kid, theta, N, X, Y, t)
        cols = [ao.window_nll_grad(kid, theta, N, X, Y[:, p], t) for p in range(P)]
        assert nll == pytest.approx(sum(c[0] for c in cols), rel=1e-13)
        np.testing.assert_allclose(g, sum(c[1] for c in cols), rtol=1e-12, atol=1e-12 * np.max(np.abs(g)))
        np.testing.assert_allclose(lml, [-c[0] for c in cols], rtol=1e-13)


def test_empty_window():
    X, Y = wm.stream(5, 2, 3, 7)
    nll, g, lml = wmo.nll_and_grad_multi(1, wm.theta_of(1, 2), 16, X, Y, 0)
    assert nll == 0.0 and g.shape == (4,) and np.all(g == 0.0) and lml.shape == (3,) and np.all(lml == 0.0)
    assert wmo.jitter(1, wm.theta_of(1, 2), 16, X, Y, 0) == 0.0


@pytest.mark.parametrize("kid,N,d", wmo.PARITY)
def test_no_parity_window_needs_jitter(kid, N, d):
    cases = [(kid, N, d, P) for P in wmo.PARITY_P] + ([wmo.PARITY_P64] if wmo.PARITY_P64[:3] == (kid, N, d) else [])
    for _, _, _, P in cases:
        X, Y, theta = wmo.parity_streams(kid, N, d, P)
        for t in wmo.parity_ticks(N):
            for w in range(wmo.PARITY_W):
                assert wmo.jitter(kid, theta, N, X[w], Y[w], t) == 0.0, (P, t, w)


@pytest.mark.parametrize("kid,N,d,P,T,seed", wmo.OPT_CASES)
def test_optimiser_cases_need_no_jitter_and_converge(kid, N, d, P, T, seed):
    """At the start and at scipy's optimum; scipy's run on the window ends with warnflag 0 within a few dozen evaluations."""
    X, Y = wm.stream(T, d, P, seed)
    th0 = wmo.opt_start(kid, d)
    assert wmo.jitter(kid, th0, N, X, Y) == 0.0
    th, lml, nev, warn = wmo.optimize_multi(kid, N, X, Y, th0)
    assert warn == 0 and 5 <= nev <= 40
    assert wmo.jitter(kid, th, N, X, Y) == 0.0
    assert lml >= -wmo.nll_and_grad_multi(kid, th0, N, X, Y)[0]
    assert lml == pytest.approx(-wmo.nll_and_grad_multi(kid, th, N, X, Y)[0], rel=1e-12)
