"""CPU checks that pin the oracle of the multi-target windows (tests/window_multi_oracle.py): against the one-factor
restatement tests/multi_oracle.py::fit_predict_multi on the window's last n samples, linearity in the targets, and the
empty-window rule."""
import numpy as np
import pytest

import multi_oracle as mto
import window_multi_oracle as wm

CASES = [(2, 16, 1), (0, 33, 2), (1, 48, 3), (3, 40, 2), (4, 24, 3)]


@pytest.mark.parametrize("kid,N,d", CASES)
def test_per_column_refit_equals_the_one_factor_restatement(kid, N, d):
    """Filling (T < N), exactly full and after two turnovers: the window is the stream's last min(T, N) samples."""
    P, M = 3, 7
    theta = wm.theta_of(kid, d)
    rng = np.random.default_rng(N)
    for T in (3, N // 2, N, 2 * N + 5):
        X, Y = wm.stream(T, d, P, 40 + N)
        Xs = wm.points_for(kid, X, T, N, M, rng)
        for noise in (True, False):
            mean, var, logml, jit = wm.sliding_window_forecast_multi(kid, theta, N, X, Y, Xs, noise, want_jitter=True)
            assert jit == 0.0
            assert mean.shape == (P, M) and var.shape == (M,) and logml.shape == (P,)
            om, ov, ol = mto.fit_predict_multi(kid, theta, X[-N:], Y[-N:].T, Xs, noise)
            em, ev, el = wm.errors(mean, var, logml, om, ov, ol)
            assert max(em, ev, el) <= 1e-10, (T, em, ev, el)


@pytest.mark.parametrize("kid,N,d", CASES)
def test_mean_is_linear_in_the_targets(kid, N, d):
    T, M, a, b = N + 9, 6, 0.7, -1.9
    theta = wm.theta_of(kid, d)
    X, Y = wm.stream(T, d, 2, 7 + N)
    Y3 = np.column_stack([Y, a * Y[:, 0] + b * Y[:, 1]])
    Xs = wm.points_for(kid, X, T, N, M, np.random.default_rng(1))
    mean, var, _ = wm.sliding_window_forecast_multi(kid, theta, N, X, Y3, Xs)
    scale = np.max(np.abs(mean))
    assert np.max(np.abs(mean[2] - (a * mean[0] + b * mean[1]))) <= 1e-10 * scale


@pytest.mark.parametrize("kid,d", [(0, 2), (2, 1), (3, 3)])
def test_empty_window_is_the_prior(kid, d):
    theta = wm.theta_of(kid, d)
    Xs = np.random.default_rng(3).normal(size=(5, d)) + 4.0
    o = wm._mod(kid)
    for noise in (True, False):
        mean, var, logml = wm.sliding_window_forecast_multi(kid, theta, 16, np.zeros((0, d)), np.zeros((0, 4)), Xs, noise)
        assert mean.shape == (4, 5) and np.all(mean == 0.0) and np.all(logml == 0.0)
        assert np.array_equal(var, o.kernel_Kdiag(kid, theta, Xs) + (theta[-1] if noise else 0.0))
