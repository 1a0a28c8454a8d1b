"""Refit oracle of the multi-target windows' summed objective (cgp_window_multi_nll_grad, cgp_window_optimize_multi): whatever
happened before, the window a stream leaves behind is its last min(T, N) samples, and the engine's value, gradient and optimum are
those of tests/multi_opt_oracle.py on these samples under the theta in force.  Test infrastructure
(tests/test_oracle_window_multi_opt.py pins it)."""
import numpy as np

import multi_opt_oracle as moo


def window_of(N, xs, Ys, t=None):
    """Samples of the window after t ticks (default: all) of the stream xs (T, d), Ys (T, P): X (n, d), Y (n, P)."""
    Ys = np.asarray(Ys, dtype=np.float64)
    t = len(Ys) if t is None else t
    xs = np.asarray(xs, dtype=np.float64)
    xs = xs.reshape(len(Ys), -1) if len(Ys) else xs.reshape(0, xs.shape[-1] if xs.ndim > 1 else 1)
    return xs[max(0, t - N):t], Ys[max(0, t - N):t]


def jitter(kid, theta, N, xs, Ys, t=None):
    """The jitter the oracle's refit of the window needs (the matrix is the same for every column): a resident window has no
    ladder, so only 0.0 is comparable."""
    Xw, Yw = window_of(N, xs, Ys, t)
    return 0.0 if len(Yw) == 0 else moo._o(kid).fit(kid, theta, Xw, Yw[:, 0]).jitter


def nll_and_grad_multi(kid, theta, N, xs, Ys, t=None):
    """-> (nll = -sum_p logml[p], gradient in natural parameters (nth,), logml (P,)); the empty window: 0, zeros, zeros."""
    Xw, Yw = window_of(N, xs, Ys, t)
    if len(Yw) == 0:
        return 0.0, np.zeros(moo.n_theta(kid, Xw.shape[1])), np.zeros(Yw.shape[1])
    return moo.nll_and_grad_multi(kid, theta, Xw, Yw.T)


# ---- the cases tests/test_gpu_window_multi_opt.py compares, shared with tests/test_oracle_window_multi_opt.py, which asserts on
# the CPU that none of them needs jitter (so the GPU test may skip nothing)
PARITY = [(2, 16, 1), (2, 17, 1), (0, 33, 2), (1, 64, 3), (1, 48, 8), (3, 40, 2), (4, 64, 3)]   # test_gpu_window_multi.py's
PARITY_P = [1, 3, 16, 17]
PARITY_P64 = (1, 48, 8, 64)   # P = 64 runs once
PARITY_W = 3
OPT_CASES = [(1, 64, 1, 3, 90, 7), (2, 48, 1, 4, 70, 7), (0, 40, 1, 17, 60, 7)]   # kid, N, d, P, T, seed


def parity_ticks(N):
    """Ticks after which the parity test compares: n = 1, 15, 16, 17 (one block, the block boundary), while filling, full, either
    side of the ring's compaction at 2 N and past it.  Uneven pushes lie between them."""
    return sorted({1, 15, 16, 17, N // 2 + 3, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 2 * N + 8})


def parity_streams(kid, N, d, P):
    """X (W, T, d), Y (W, T, P), theta: test_gpu_window_multi.py's streams of the case."""
    import window_multi_oracle as wm
    T = 2 * N + 8
    Xw, Yw = zip(*[wm.stream(T, d, P, 1000 * kid + N + 17 * w) for w in range(PARITY_W)])
    return np.stack(Xw), np.stack(Yw), wm.theta_of(kid, d)


def opt_start(kid, d):
    import window_multi_oracle as wm
    return wm.theta_of(kid, d) if kid == 2 else np.concatenate([[0.05], np.ones(moo.n_theta(kid, d) - 2), [0.01]])


def optimize_multi(kid, N, xs, Ys, theta0, t=None, max_evals=1000):
    """m.optimize() of the multi-column model on the window: (theta, sum_p logml, evaluations, warnflag)."""
    Xw, Yw = window_of(N, xs, Ys, t)
    return moo.optimize_multi(kid, Xw, Yw.T, theta0, max_evals)
