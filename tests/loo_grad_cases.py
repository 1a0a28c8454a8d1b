"""The windows the GPU tests of the leave-one-out objective compare with tests/loo_grad_oracle.py, in one place so that
tests/test_oracle_loo_grad.py can hold every one of them to the condition the 1e-6 bar rests on: no jitter, and the float64 closed
form within 1e-8 of max|grad| of the central difference.  Recipes are tests/test_gpu_loo.py's."""
import numpy as np

import corenav_gp_amd.synth as synth

KERNEL_SHAPES = [(0, 3), (1, 3), (1, 8), (2, 1), (3, 3), (4, 3)]   # (kernel id, d) at N = 130
EDGE_N, EDGE_D = [1, 2, 127, 128, 129, 257], [1, 3, 6]
SCHEDULES = [(3, 257), (30, 257), (50, 257), (512, 130)]   # test_gpu_loo.py's: latency, mid-size, throughput, full batch
# the optimiser: d = 1 on the time base, from all-ones: (kernel id, N, seed, theta compared).  Seeds chosen on the CPU
# (tests/test_oracle_loo_grad.py::test_optimiser_windows holds them to it): scipy ends with warnflag 0 on every one; theta is
# compared where every optimal parameter is > 1e-6, else the window is held to the value bar alone.
OPT_WINDOWS = [(0, 130, 43, True), (1, 130, 43, True), (2, 134, 43, True), (3, 130, 43, True), (4, 130, 43, True)]


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def window(N, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [rng.normal(size=N) for _ in range(d - 1)]), y


def problem(B, N, d, kid, seed):
    rng = np.random.default_rng(seed)
    Xw, yw = zip(*[window(N, d, seed + 17 * b, tick0=11 + b) for b in range(B)])
    theta = np.tile(theta_of(kid, d), (B, 1))
    theta[:, 0] *= 1.0 + 0.2 * rng.random(B)
    return np.stack(Xw), np.stack(yw), theta


def edge_kernel(N, d):
    return (1, 3, 4, 0)[(N + d) % 4] if d > 1 else (2, 0, 3)[N % 3]


def kernel_problem(kid, d):
    return problem(2, 130, d, kid, 300 + 10 * kid + d)


def edge_problem(N, d):
    return problem(2, N, d, edge_kernel(N, d), 100 * N + d)


def schedule_problem(B, N):
    """Fit 1's window also sits in the last slot."""
    X, y, theta = problem(B, N, 3, 1, 7 + B)
    X[-1], y[-1], theta[-1] = X[1], y[1], theta[1]
    return X, y, theta


def schedule_checked(B):
    return sorted({0, 1, B // 2, B - 1})


def compared_windows():
    """(label, kid, theta, X, y) of every fit a GPU test holds to the oracle at 1e-6."""
    for kid, d in KERNEL_SHAPES:
        X, y, th = kernel_problem(kid, d)
        for b in range(2):
            yield f"kernel {kid} d {d} fit {b}", kid, th[b], X[b], y[b]
    for N in EDGE_N:
        for d in EDGE_D:
            X, y, th = edge_problem(N, d)
            for b in range(2):
                yield f"edge N {N} d {d} fit {b}", edge_kernel(N, d), th[b], X[b], y[b]
    for B, N in SCHEDULES:
        X, y, th = schedule_problem(B, N)
        for b in schedule_checked(B):
            yield f"schedule {B} x {N} fit {b}", 1, th[b], X[b], y[b]
