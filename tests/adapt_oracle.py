"""Refit oracle of the sliding windows under a theta that changes mid-stream (cgp_window_set_theta, cgp_window_nll_grad,
cgp_window_optimize), on top of oracle/gp_oracle.py: whatever happened before, the window after t ticks is the last min(t, N)
samples, and everything the engine reports is a refit of those samples under the theta in force.  Test infrastructure
(tests/test_oracle_window_adapt.py checks it against sliding_window_stream)."""
import numpy as np

from oracle import gp_oracle as go


def window_of(N, xs, ys, t):
    """Samples of the window after t ticks of the stream (xs, ys)."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1)
    return xs[max(0, t - N):t], np.asarray(ys, dtype=np.float64)[max(0, t - N):t]


def window_logml(kernel_id, theta, N, xs, ys, t):
    Xw, yw = window_of(N, xs, ys, t)
    return 0.0 if len(yw) == 0 else go.fit(kernel_id, theta, Xw, yw).logml


def window_nll_grad(kernel_id, theta, N, xs, ys, t):
    Xw, yw = window_of(N, xs, ys, t)
    if len(yw) == 0:
        return 0.0, np.zeros(go.n_theta(kernel_id, Xw.shape[1]))
    return go.nll_and_grad(kernel_id, theta, Xw, yw)


def stream_ticks(kernel_id, theta, N, xs, ys, t0, t1, include_noise=True):
    """Outputs of ticks t0 .. t1 - 1 of the stream (xs, ys) through a window of length N when `theta` is in force for those
    ticks, whatever theta the earlier ticks ran under: one-step-ahead mean / variance of sample t from the window before it
    (the oldest sample of a full window leaves first) and logML of the window after it.  Every tick is two refits from scratch."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1)
    ys = np.asarray(ys, dtype=np.float64)
    pm, pv, lm = np.zeros(t1 - t0), np.zeros(t1 - t0), np.zeros(t1 - t0)
    for i, t in enumerate(range(t0, t1)):
        lo = max(0, t - N + 1) if t >= N else 0
        if t == lo:
            pm[i] = 0.0
            pv[i] = go.kernel_Kdiag(kernel_id, theta, xs[t:t + 1])[0] + (go.noise_var(kernel_id, theta) if include_noise else 0.0)
        else:
            mu, var = go.predict(go.fit(kernel_id, theta, xs[lo:t], ys[lo:t]), xs[t:t + 1], include_noise)
            pm[i], pv[i] = mu[0], var[0]
        lm[i] = go.fit(kernel_id, theta, xs[lo:t + 1], ys[lo:t + 1]).logml
    return pm, pv, lm
