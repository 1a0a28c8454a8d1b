"""Oracle of the windows' leave-one-out objective (cgp_window_loo_nll_grad, cgp_window_optimize_loo) and the cases its GPU tests
compare: whatever happened before, the window after t ticks is the last min(t, N) samples in window order (adapt_oracle.window_of),
and the objective is tests/loo_grad_oracle.py's on those samples at the theta in force; the empty window gives (0, zeros).  The
case lists live here so that tests/test_oracle_window_loo_grad.py can hold every compared window to the condition the 1e-6 bar
rests on: no jitter, and the float64 closed form within 1e-8 of max|grad| of the central difference.  Recipes (stream, theta_of)
are tests/test_gpu_window_loo.py's."""
import functools

import numpy as np

from adapt_oracle import window_of
import loo_grad_oracle as lgo
from test_gpu_window_loo import stream, theta_of

# (kernel id, N, d): the 16-row block edges, a capacity that is no multiple of 16, the 64-row super-tile edge with one live row in
# the second super-tile (ticks 65 at N = 80), d = 8, every kernel id
RING_SHAPES = [(2, 16, 1), (2, 17, 1), (0, 33, 1), (1, 33, 2), (1, 64, 3), (1, 48, 8), (3, 40, 2), (4, 64, 3), (1, 80, 2)]
RING_W = 3
# the optimiser: (kernel id, N, T, theta0, scipy's evaluations); d = 1, stream(T, 1, 7)
OPT_CASES = [(1, 64, 90, (0.05, 1.0, 0.01), 23), (0, 40, 60, (0.05, 1.0, 0.01), 20), (2, 48, 70, (0.5, 30.0, 0.01, 0.002), 34)]
FIVE = [(0, 1), (1, 3), (2, 1), (3, 2), (4, 6)]   # (kernel id, d) of the five-window cases, N = 40 (SE-iso at d = 1: the
# central difference of this recipe at d = 2 is itself 1.4e-8 ... 4.7e-8 off)
FIVE_N, FIVE_T = 40, (21, 53)
BIG_THETA = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])


def window_nlpd_and_grad(kid, theta, N, xs, ys, t):
    """(nlpd, grad, logml, jitter) of the window after t ticks of the stream (xs, ys)."""
    Xw, yw = window_of(N, xs, ys, t)
    if len(yw) == 0:
        return 0.0, np.zeros(lgo.n_theta(kid, Xw.shape[1])), 0.0, 0.0
    return lgo.nlpd_and_grad(kid, theta, Xw, yw)


def ring_ticks(N):
    t = {1, 15, 16, 17, N // 2 + 3, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 2 * N + 8}
    if N > 65:
        t |= {63, 64, 65}
    return sorted(t)


@functools.lru_cache(maxsize=None)
def ring_case(kid, N, d):
    """Three windows: window w has seed 1000 kid + N + 17 w, tick0 = 11 + 3 w and theta[0] scaled by 1 + 0.1 w."""
    T = ring_ticks(N)[-1]
    Xw, yw = zip(*[stream(T, d, 1000 * kid + N + 17 * w, tick0=11 + 3 * w) for w in range(RING_W)])
    theta = np.tile(theta_of(kid, d), (RING_W, 1))
    theta[:, 0] *= 1.0 + 0.1 * np.arange(RING_W)
    return np.stack(Xw), np.stack(yw), theta


@functools.lru_cache(maxsize=None)
def five_case(kid, d):
    """Five windows of N = 40, each with its own stream and theta (tests/test_gpu_window_loo.py's recipe)."""
    W, T = 5, FIVE_T[-1]
    Xw, yw = zip(*[stream(T, d, 100 * kid + w, tick0=11 + 3 * w) for w in range(W)])
    theta = np.tile(theta_of(kid, d), (W, 1))
    theta[:, 0] *= 1.0 + 0.1 * np.arange(W)
    return np.stack(Xw), np.stack(yw), theta


@functools.lru_cache(maxsize=None)
def big_case(N):
    """(N, T, kid, theta, X, y): N = 512 after 700 ticks of stream(700, 3, 7); N = 700 after 1 500 ticks of stream(1500, 3, 700)."""
    T, seed = {512: (700, 7), 700: (1500, 700)}[N]
    X, y = stream(T, 3, seed)
    return N, T, 1, BIG_THETA, X, y


def ring_label(kid, N, d, w, t):
    return f"ring kid {kid} N {N} d {d} window {w} t {t}"


def compared_windows(big=True):
    """(label, kid, theta, X, y) of every window a GPU test holds to the oracle at 1e-6."""
    for kid, N, d in RING_SHAPES:
        X, y, th = ring_case(kid, N, d)
        for t in ring_ticks(N):
            for w in range(RING_W):
                yield (ring_label(kid, N, d, w, t), kid, th[w], *window_of(N, X[w], y[w], t))
    for kid, d in FIVE:
        X, y, th = five_case(kid, d)
        for t in FIVE_T:
            for w in range(5):
                yield (f"five kid {kid} d {d} window {w} t {t}", kid, th[w], *window_of(FIVE_N, X[w], y[w], t))
    if big:
        for N in (512, 700):
            _, T, kid, th, X, y = big_case(N)
            yield (f"big N {N}", kid, th, *window_of(N, X, y, T))


def opt_case(kid, N, T):
    X, y = stream(T, 1, 7)
    return window_of(N, X, y, T)
