"""sliding_window_forecast (the refit oracle of cgp_window_predict) against sliding_window_stream: the forecast at the next
sample's input, made after dropping the oldest sample by hand, is that tick's one-step-ahead mean / variance."""
import numpy as np
import pytest

from oracle import gp_oracle as go
from forecast_oracle import sliding_window_forecast
import corenav_gp_amd.synth as synth


def stream(T, d, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + T, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)]), y


@pytest.mark.parametrize("kid,N,d,theta", [(2, 12, 1, [0.5, 30.0, 0.01, 0.002]), (0, 9, 2, [0.02, 1.0, 1e-3]),
                                           (1, 20, 3, [0.02, 0.8, 1.2, 1.6, 1e-3])])
@pytest.mark.parametrize("noise", [True, False])
def test_forecast_at_the_next_input_is_the_streams_one_step_prediction(kid, N, d, theta, noise):
    T = 3 * N + 2
    X, y = stream(T, d, 10 * N + d)
    theta = np.array(theta)
    pm, pv, _ = go.sliding_window_stream(kid, theta, N, X, y, include_noise=noise)
    for t in range(T):
        lo = max(0, t - N + 1) if t >= N else 0     # a full window drops its oldest sample before it predicts
        mu, var = sliding_window_forecast(kid, theta, N, X[lo:t], y[lo:t], X[t:t + 1], include_noise=noise)
        assert mu.shape == var.shape == (1,)
        assert mu[0] == pytest.approx(pm[t], rel=1e-12, abs=1e-15) and var[0] == pytest.approx(pv[t], rel=1e-12)


def test_forecast_keeps_the_last_N_samples_and_answers_an_empty_stream_with_the_prior():
    X, y = stream(40, 1, 3)
    theta = np.array([0.5, 30.0, 0.01, 0.002])
    Xs = X[-1, 0] + 1.0 + np.arange(25.0)[:, None]
    mu, var = sliding_window_forecast(2, theta, 16, X, y, Xs)
    emu, evar = go.predict(go.fit(2, theta, X[-16:], y[-16:]), Xs)
    assert np.array_equal(mu, emu) and np.array_equal(var, evar)
    mu0, var0 = sliding_window_forecast(2, theta, 16, X[:0], y[:0], Xs, include_noise=False)
    assert np.all(mu0 == 0.0) and np.array_equal(var0, go.kernel_Kdiag(2, theta, Xs))
    assert np.allclose(sliding_window_forecast(2, theta, 16, X[:0], y[:0], Xs)[1], var0 + theta[3], rtol=1e-15)
