"""CPU tests of tests/window_loo_grad_oracle.py: the condition every window a GPU test of cgp_window_loo_nll_grad compares must
meet (no jitter; the closed form within 1e-8 of max|grad| of the central difference, tests/test_oracle_loo_grad.py's condition),
the empty window, and what the optimiser cases rest on: scipy on the oracle ends each with warnflag 0 after the recorded number of
evaluations and no trial point needs jitter -- the window route has no ladder, the batch route it is compared with has one."""
import numpy as np
import pytest

import loo_grad_oracle as lgo
import window_loo_grad_oracle as wo

SELF = 1e-8   # the oracle against its independent check, of max|grad|


def rel(g, want):
    return float(np.max(np.abs(g - want)) / np.max(np.abs(want)))


def test_empty_window_and_window_order():
    X, y = wo.stream(30, 2, 5)
    th = wo.theta_of(1, 2)
    f, g, lml, jit = wo.window_nlpd_and_grad(1, th, 8, X, y, 0)
    assert f == 0.0 and lml == 0.0 and jit == 0.0 and np.array_equal(g, np.zeros(4))
    f, g, _, _ = wo.window_nlpd_and_grad(1, th, 8, X, y, 19)
    f2, g2, _, _ = lgo.nlpd_and_grad(1, th, X[11:19], y[11:19])
    assert f == f2 and np.array_equal(g, g2)
    f, _, _, _ = wo.window_nlpd_and_grad(1, th, 8, X, y, 5)
    assert f == lgo.nlpd_and_grad(1, th, X[:5], y[:5])[0]


def test_case_lists():
    assert wo.ring_ticks(16) == [1, 11, 15, 16, 17, 31, 32, 33, 40]
    assert {63, 64, 65} <= set(wo.ring_ticks(80)) and 64 not in wo.ring_ticks(40)
    assert all(kid != 0 or d == 1 for kid, _, d in wo.RING_SHAPES) and all(kid != 0 or d == 1 for kid, d in wo.FIVE)
    assert {k for k, _, _ in wo.RING_SHAPES} == {0, 1, 2, 3, 4}
    X, y, th = wo.ring_case(1, 33, 2)
    assert X.shape == (3, 74, 2) and th[2, 0] == pytest.approx(1.2 * th[0, 0]) and not np.array_equal(y[0], y[1])


def test_every_compared_small_window_meets_the_condition():
    worst = 0.0
    for label, kid, th, X, y in wo.compared_windows(big=False):
        _, g, _, jit = lgo.nlpd_and_grad(kid, th, X, y)
        e = rel(g, lgo.central_difference(kid, th, X, y))
        worst = max(worst, e)
        assert jit == 0.0 and e <= SELF, (label, jit, e)
    print("worst", worst)


@pytest.mark.parametrize("N", [512, 700])
def test_the_two_long_windows_meet_the_condition(N):
    _, T, kid, th, X, y = wo.big_case(N)
    Xw, yw = wo.window_of(N, X, y, T)
    f, g, _, jit = lgo.nlpd_and_grad(kid, th, Xw, yw)
    e = rel(g, lgo.central_difference(kid, th, Xw, yw))
    print(N, f, jit, e)
    assert len(yw) == N and jit == 0.0 and e <= SELF
    if N == 512:
        assert f == pytest.approx(249.16, abs=5e-3)


@pytest.mark.parametrize("kid,N,T,theta0,evals", wo.OPT_CASES)
def test_optimiser_cases(monkeypatch, kid, N, T, theta0, evals):
    Xw, yw = wo.opt_case(kid, N, T)
    jitters = []
    inner = lgo.nlpd_and_grad

    def recording(*a):
        out = inner(*a)
        jitters.append(out[3])
        return out
    monkeypatch.setattr(lgo, "nlpd_and_grad", recording)
    th, lpd, nev, warn = lgo.optimize_loo(kid, Xw, yw, theta0=np.array(theta0))
    print(kid, N, T, th, lpd, nev, warn, max(jitters))
    assert len(yw) == N and warn == 0 and nev == evals and len(jitters) == nev and max(jitters) == 0.0
    assert np.min(th) >= 7.5e-4 * (1 - 1e-2)
