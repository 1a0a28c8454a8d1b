"""The test-support oracle of the windows under a changing theta (tests/adapt_oracle.py) against sliding_window_stream: with one
theta it is that stream, and after a change of theta it is that stream restarted under the new theta on the window's samples."""
import numpy as np
import pytest

from oracle import gp_oracle as go
from adapt_oracle import stream_ticks, window_logml, window_nll_grad, window_of
import corenav_gp_amd.synth as synth


def _stream(T, d, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + T, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)]), y


@pytest.mark.parametrize("kid,N,d", [(2, 12, 1), (0, 9, 2), (1, 16, 3)])
def test_one_theta_is_the_sliding_window_stream(kid, N, d):
    T = 3 * N + 2
    X, y = _stream(T, d, N)
    theta = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]), 1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]
    for noise in (True, False):
        ref = go.sliding_window_stream(kid, theta, N, X, y, include_noise=noise)
        got = stream_ticks(kid, theta, N, X, y, 0, T, include_noise=noise)
        for a, b in zip(got, ref):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("t0", [5, 12, 20, 31])
def test_theta_changed_mid_stream_is_the_stream_restarted_on_the_windows_samples(t0):
    kid, N, d, T = 1, 12, 2, 40
    X, y = _stream(T, d, 77)
    th2 = np.array([0.05, 0.7, 1.9, 4e-3])
    got = stream_ticks(kid, th2, N, X, y, t0, T)
    Xw, yw = window_of(N, X, y, t0)
    n = len(yw)
    assert n == min(t0, N)
    # the restarted stream first re-reads the window's own samples, then the ticks that follow the change
    ref = go.sliding_window_stream(kid, th2, N, np.vstack([Xw, X[t0:]]), np.concatenate([yw, y[t0:]]))
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a, b[n:], rtol=1e-12, atol=1e-15)
    assert window_logml(kid, th2, N, X, y, t0) == pytest.approx(ref[2][n - 1], rel=1e-12)
    nll, g = window_nll_grad(kid, th2, N, X, y, t0)
    assert nll == pytest.approx(-ref[2][n - 1], rel=1e-12) and g.shape == (4,)


def test_empty_window():
    X, y = _stream(4, 1, 1)
    assert window_logml(2, np.array([0.5, 30.0, 0.01, 0.002]), 8, X, y, 0) == 0.0
    nll, g = window_nll_grad(2, np.array([0.5, 30.0, 0.01, 0.002]), 8, X, y, 0)
    assert nll == 0.0 and np.all(g == 0.0)
