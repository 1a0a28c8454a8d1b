"""CPU tests of tests/loo_grad_oracle.py, the oracle of the leave-one-out objective's gradient: the closed form against central
differences of loo_oracle.loo, of the brute-force definition (N refits) and against 50-digit values; the condition every window a
GPU test compares must meet; the optimiser windows."""
import numpy as np
import pytest

from conftest import load_golden
import loo_oracle as lo
import loo_grad_oracle as lgo
import loo_grad_cases as lc

SELF = 1e-8   # the oracle against its independent checks, of max|grad|


def rel(g, want):
    return float(np.max(np.abs(g - want)) / np.max(np.abs(want)))


def test_value_is_loo_oracles_negated():
    X, y, th = lc.problem(1, 60, 2, 1, 3)
    f, _, lml, jit = lgo.nlpd_and_grad(1, th[0], X[0], y[0])
    want = lo.loo(1, th[0], X[0], y[0])
    assert f == -want.lpd_sum and lml == want.logml and jit == 0.0


@pytest.mark.parametrize("kid,d", [(0, 1), (0, 2), (1, 3), (2, 1), (3, 2), (4, 1)])
def test_closed_form_against_the_brute_force_definition(kid, d):
    """N = 12: central differences of N refits on N - 1 samples each."""
    X, y, th = lc.problem(1, 12, d, kid, 50 + kid)
    _, g, _, jit = lgo.nlpd_and_grad(kid, th[0], X[0], y[0])
    cd = lgo.central_difference(kid, th[0], X[0], y[0], value=lambda t: lo.loo_brute(kid, t, X[0], y[0]).lpd_sum)
    print(kid, d, rel(g, cd))
    assert jit == 0.0 and rel(g, cd) <= SELF


@pytest.mark.parametrize("src,pin", [("mp_rbfbrownian_n134", "loo_grad_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_grad_mp_m32_n134"),
                                     ("matern_mp_m52_n134", "loo_grad_mp_m52_n134")])
def test_closed_form_against_50_digits(src, pin):
    g, p = load_golden(src), load_golden(pin)
    f, grad, _, jit = lgo.nlpd_and_grad(int(g["kernel_id"]), g["theta"], g["X"], g["y"])
    print(pin, abs(f - float(p["nlpd"])) / abs(float(p["nlpd"])), rel(grad, p["grad"]))
    assert jit == 0.0 and abs(f - float(p["nlpd"])) <= 1e-9 * abs(float(p["nlpd"])) and rel(grad, p["grad"]) <= SELF


def test_every_compared_window_meets_the_condition():
    """No jitter, and the closed form within 1e-8 of max|grad| of the central difference: the GPU tests' 1e-6 then measures the
    engine, not the oracle."""
    worst = 0.0
    for label, kid, th, X, y in lc.compared_windows():
        _, g, _, jit = lgo.nlpd_and_grad(kid, th, X, y)
        e = rel(g, lgo.central_difference(kid, th, X, y))
        worst = max(worst, e)
        assert jit == 0.0 and e <= SELF, (label, jit, e)
    print("worst", worst)


@pytest.mark.parametrize("kid,N,seed,theta_compared", lc.OPT_WINDOWS)
def test_optimiser_windows(kid, N, seed, theta_compared):
    """scipy ends with warnflag 0; theta is compared on the GPU exactly where every optimal parameter is > 1e-6."""
    X, y = lc.window(N, 1, seed)
    th, lpd, nev, warn = lgo.optimize_loo(kid, X, y)
    print(kid, th, lpd, nev)
    assert warn == 0 and nev < 1000 and theta_compared == bool(np.all(th > 1e-6))
    assert lpd == pytest.approx(-lgo.nlpd_and_grad(kid, th, X, y)[0], rel=1e-12)
    assert lpd > -lgo.nlpd_and_grad(kid, np.ones(len(th)), X, y)[0]
