"""Refit oracle of the sliding windows' predictive gradients (cgp_window_predict_gradients), on top of tests/pgrad_oracle.py:
the samples a stream leaves in a window of length N, fitted from scratch, and pgrad_oracle.predictive_gradients at Xs; the prior
rule for an empty stream (dmean 0, dvar = d k(x*, x*) / dx*).  Test infrastructure: the GPU tests, the fuzz script and the C
caller's test compare against it; tests/test_oracle_window_pgrad.py checks it against central differences."""
import numpy as np

import pgrad_oracle as po


def window_fit(kernel_id, theta, N, xs, ys):
    """The fit of the last min(len(ys), N) samples of the stream (a go.Fit); None for an empty stream."""
    if len(ys) == 0:
        return None
    xs = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1)
    return po.fit(kernel_id, theta, xs[-N:], np.asarray(ys, dtype=np.float64)[-N:])


def prior_gradients(kernel_id, theta, Xs):
    """What an empty window answers: dmean = 0, dvar = d k(x*, x*) / dx* (sigma_r^2 sigma_b^2 sign(x*) for id 2, else zero)."""
    Xs = po._as2d(Xs)
    _, dkss = po.dK_dxs(kernel_id, theta, Xs[:1], Xs)
    return np.zeros(Xs.shape), dkss


def sliding_window_gradients(kernel_id, theta, N, xs, ys, Xs):
    """(dmean, dvar), each (M, d), at Xs from the window a stream (xs, ys) leaves behind."""
    Xs = po._as2d(Xs)
    f = window_fit(kernel_id, theta, N, xs, ys)
    if f is None:
        return prior_gradients(kernel_id, theta, Xs)
    return po.predictive_gradients(f, Xs)
