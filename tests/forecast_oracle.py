"""Refit oracle of the sliding windows' forecast (cgp_window_predict), on top of oracle/gp_oracle.py: the samples a stream
leaves in a window of length N, fitted from scratch, predicted at Xs.  Test infrastructure (the GPU tests, the fuzz script and
the C caller's test compare against it; tests/test_oracle_window_forecast.py checks it against sliding_window_stream)."""
import numpy as np

from oracle import gp_oracle as go


def sliding_window_forecast(kernel_id, theta, N, xs, ys, Xs, include_noise=True):
    """Forecast at Xs from the window a stream (xs, ys) leaves behind: the last min(len(ys), N) samples refitted from
    scratch; the prior for an empty stream.  Returns (mean, var)."""
    Xs = np.asarray(Xs, dtype=np.float64)
    if Xs.ndim == 1:
        Xs = Xs[:, None]
    if len(ys) == 0:
        return np.zeros(len(Xs)), go.kernel_Kdiag(kernel_id, theta, Xs) + (go.noise_var(kernel_id, theta) if include_noise else 0.0)
    xs = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1)
    return go.predict(go.fit(kernel_id, theta, xs[-N:], np.asarray(ys, dtype=np.float64)[-N:]), Xs, include_noise)
