"""The refit oracle of the sliding windows' predictive gradients (tests/window_pgrad_oracle.py) against central differences of
pgrad_oracle.unclipped_mean_var on the same window, at the step and the bar of tests/test_oracle_pgrad.py (h = 1e-5, 2e-6 of the
largest gradient entry): ids 0 - 4, a window still filling and a full one that has slid; for id 2 points inside the window off
the ticks and after it under the differences, and points ON the ticks (ties |x*| = |x_i|, where the derivative of min jumps)
against the one-sided limit.  The empty-window rule: dmean 0, dvar = d k(x*, x*) / dx*, with the sign at x* < 0, = 0, > 0."""
import numpy as np
import pytest

import pgrad_oracle as po
import window_pgrad_oracle as wo
from test_oracle_pgrad import theta_of, window


def stream(T, d, seed):
    return window(T, d, seed)


def central(f, Xs, h=1e-5):
    d = Xs.shape[1]
    fm, fv = np.empty(Xs.shape), np.empty(Xs.shape)
    for q in range(d):
        e = np.zeros(d)
        e[q] = h
        mp, vp = po.unclipped_mean_var(f, Xs + e)
        mm, vm = po.unclipped_mean_var(f, Xs - e)
        fm[:, q], fv[:, q] = (mp - mm) / (2 * h), (vp - vm) / (2 * h)
    return fm, fv


def points(kid, Xw, M, rng):
    """Xw: the samples in the window.  id 2: after the window on the ticks, and inside it off the ticks."""
    if kid == 2:
        after = Xw[-1, 0] + 1.0 + np.arange(M // 2, dtype=np.float64)
        inside = Xw[rng.integers(0, max(len(Xw) - 1, 1), size=M - M // 2), 0] + rng.uniform(0.2, 0.8, size=M - M // 2)
        return np.concatenate([after, inside])[:, None]
    return Xw[rng.integers(0, len(Xw), size=M)] + 0.3 * rng.normal(size=(M, Xw.shape[1]))


@pytest.mark.parametrize("kid,N,d", [(0, 40, 3), (1, 48, 6), (2, 60, 1), (3, 40, 2), (4, 50, 4)])
@pytest.mark.parametrize("t_of_n", [lambda N: N // 2 + 1, lambda N: 2 * N + 5], ids=["filling", "full"])
def test_refit_oracle_against_central_differences(kid, N, d, t_of_n):
    t = t_of_n(N)
    X, y = stream(t, d, seed=kid + N)
    theta = theta_of(kid, d)
    rng = np.random.default_rng(10 * kid + t)
    Xw = X[-N:]
    assert len(Xw) == min(t, N)
    Xs = points(kid, Xw, 12, rng)
    dmean, dvar = wo.sliding_window_gradients(kid, theta, N, X, y, Xs)
    assert dmean.shape == dvar.shape == (12, d)
    f = wo.window_fit(kid, theta, N, X, y)
    assert len(f.X) == min(t, N) and np.array_equal(f.X, Xw)
    fm, fv = central(f, Xs)
    em = np.max(np.abs(dmean - fm)) / np.max(np.abs(dmean))
    ev = np.max(np.abs(dvar - fv)) / np.max(np.abs(dvar))
    print(f"kid {kid} t {t}: dmean {em:.3g} dvar {ev:.3g}")
    assert em < 2e-6 and ev < 2e-6, (em, ev)


def test_brownian_points_on_the_ticks_inside_the_window():
    """At a tie the oracle's gradient is the limit from the side where |x*| is the larger: central differences of a point
    moved 1e-3 beyond the tick (no tie inside the stencil) converge to it; the differences astride the tick do not."""
    N, t = 40, 90
    X, y = stream(t, 1, seed=5)
    theta = theta_of(2, 1)
    f = wo.window_fit(2, theta, N, X, y)
    ties = X[-N:][[3, 17, 38]]
    dm, dv = wo.sliding_window_gradients(2, theta, N, X, y, ties)
    assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
    dm_b, dv_b = wo.sliding_window_gradients(2, theta, N, X, y, ties + 1e-3)
    fm, fv = central(f, ties + 1e-3)
    assert np.max(np.abs(dm_b - fm)) < 2e-6 * np.max(np.abs(dm_b)) and np.max(np.abs(dv_b - fv)) < 2e-6 * np.max(np.abs(dv_b))
    # continuity from above: the tie's value is within the slope's change over 1e-3 of the value just beyond it
    assert np.max(np.abs(dm - dm_b)) < 1e-2 * np.max(np.abs(dm)) and np.max(np.abs(dv - dv_b)) < 1e-2 * np.max(np.abs(dv))
    dm_a, _ = wo.sliding_window_gradients(2, theta, N, X, y, ties - 1e-3)
    assert np.max(np.abs(dm - dm_a)) > 10 * np.max(np.abs(dm - dm_b))    # the other side carries the bracket


@pytest.mark.parametrize("kid,d", [(0, 3), (1, 2), (2, 1), (3, 4), (4, 1)])
def test_empty_window_rule(kid, d):
    theta = theta_of(kid, d)
    rng = np.random.default_rng(kid)
    Xs = rng.normal(size=(7, d))
    Xs[0], Xs[1], Xs[2] = -2.5, 0.0, 3.0
    dmean, dvar = wo.sliding_window_gradients(kid, theta, 16, np.empty((0, d)), np.empty(0), Xs)
    assert dmean.shape == dvar.shape == (7, d) and np.all(dmean == 0.0)
    if kid == 2:
        np.testing.assert_array_equal(dvar[:3, 0], theta[0] * theta[2] * np.array([-1.0, 0.0, 1.0]))
        np.testing.assert_array_equal(dvar[:, 0], theta[0] * theta[2] * np.sign(Xs[:, 0]))
        # it is the derivative of the prior variance sigma_r^2 sigma_b^2 |x*| away from the origin
        kss = lambda x: po.go.kernel_Kdiag(2, theta, x)
        num = (kss(Xs[[0, 2]] + 1e-6) - kss(Xs[[0, 2]] - 1e-6)) / 2e-6
        np.testing.assert_allclose(dvar[[0, 2], 0], num, rtol=1e-8)
    else:
        assert np.all(dvar == 0.0)
