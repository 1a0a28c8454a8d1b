"""Inputs and oracle of the FAILURE path (include/corenav_gp.h: a positive return or `info` is the LAPACK-style 1-based index of
the first non-positive pivot): windows whose factorisation fails at a CHOSEN pivot, by a margin no rounding can move, and the
plain reference that says so.  Test infrastructure: tests/test_oracle_failure.py establishes the margin of every case on the
CPU, tests/test_gpu_failure_paths.py runs the same cases through the engine.

Construction.  The inputs are points of an integer lattice, four length-scales apart (sigma_f^2 = 1: every off-diagonal
covariance of the squared-exponential kernel is <= e^-8), the noise variance is NEGATIVE (sigma_n^2 + 1e-8 = -0.05: every
diagonal entry of Ky is 0.95), and the input of row p is overwritten with that of an earlier row q: the 2 x 2 block of the pair
is [[0.95, 1], [1, 0.95]], so the pivot of row p is about 0.95 - 1 / 0.95 = -0.10 while every pivot before it stays about 0.95.
The largest rung of GPy's jitter ladder adds 1e-2 mean(diag) < 0.05: the host entry points fail at the same pivot on every rung.
RBF x Brownian (d = 1; diag = sigma_rbf^2 sigma_b^2 x_i) takes raw ticks in a narrow band, x_i = 2000 + 4 ell i, and a shift of
-0.05 mean(diag) on the noise: the healthy pivots stay above 1870 a, the failing one is about -250 a (a = sigma_rbf^2 sigma_b^2).

rung_window: the same lattice with a shift of a few 1e-5 instead of 0.05.  K itself is positive semi-definite with an exact
zero eigenvalue on the duplicated pair, so Ky + j I is positive definite exactly when j exceeds the shift: the rung of the
ladder that is needed is chosen by the shift, whichever pivot the pair sits at."""
import itertools

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go
import matern_oracle as mo

SPACING = 4.0                       # lattice spacing in length-scales
ELL3 = (0.5, 1.0, 2.0)              # ARD length-scales of the d = 3 lattice (the scaled coordinates are what is 4 apart)
SHIFT = 0.05                        # sigma_n^2 + 1e-8 = -SHIFT * mean(diag K): beyond the ladder's last rung (1e-2)
MARGIN = 1e-3                       # the condition on every case, in units of mean(diag Ky)
BROWN_X0, BROWN_A = 2000.0, (0.5, 0.01)   # first tick; sigma_rbf^2, sigma_b^2
RUNGS = tuple(1e-6 * 10.0 ** k for k in range(5))   # GPy jitchol: mean(diag) * 1e-6 * 10^k


def kernel_K(kid, theta, X):
    return (mo.kernel_K if kid in mo.KERNELS else go.kernel_K)(kid, theta, X)


def ky_of(kid, theta, X, jitter=0.0):
    """Ky = K + (sigma_n^2 + 1e-8 + jitter) I, the matrix every entry point factors."""
    Ky = np.array(kernel_K(kid, theta, np.asarray(X, dtype=np.float64)), dtype=np.float64)
    Ky[np.diag_indices(len(Ky))] += float(theta[-1]) + go.GPY_DIAG_EPS + jitter
    return Ky


def first_bad_pivot(Ky):
    """Plain unblocked (left-looking) Cholesky in numpy.longdouble.  Returns (info, pivots): info the 1-based index of the first
    non-positive pivot (0: none), pivots the Schur-complement diagonal up to and including that row, as float64."""
    A = np.asarray(Ky, dtype=np.longdouble)
    N = len(A)
    L = np.zeros((N, N), dtype=np.longdouble)
    piv = np.zeros(N)
    for j in range(N):
        pj = A[j, j] - np.dot(L[j, :j], L[j, :j])
        piv[j] = float(pj)
        if not pj > 0:
            return j + 1, piv[:j + 1]
        L[j, j] = np.sqrt(pj)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0, piv


def lattice_points(N, d, start=0):
    """Points [start, start + N) of the lattice, in the order of itertools.product (d = 3: 7 x 7 x 6 = 294 points)."""
    if d == 3:
        P = np.array(list(itertools.islice(itertools.product(range(7), range(7), range(6)), start, start + N)), dtype=np.float64)
    else:
        assert d == 1
        P = np.arange(start, start + N, dtype=np.float64)[:, None]
    assert len(P) == N
    return P


def _targets(N, seed):
    return 0.1 * np.sin(np.arange(N) / 5.0) + 0.03 * np.random.default_rng(seed).normal(size=N)


def lattice_window(kid, N, d, p=None, q=None, seed=0, shift=SHIFT, start=0):
    """X (N, d), y (N,), theta of kernel `kid` (1 SE-ARD, 4 Matern 5/2: [1, ell.., noise]; 2 RBF x Brownian: [a0, 1, a1, noise])
    with sigma_n^2 + 1e-8 = -shift * mean(diag K).  p given: X[p] = X[q], q < p (default p // 2) -- the fit fails at 0-based row
    p.  p None: no duplicate, the window factors (every pivot about (1 - shift) of the diagonal).  start: the window is points
    [start, start + N) of the lattice (what a resident window holds after start + N pushes)."""
    P = lattice_points(N, d, start)
    if kid == go.KERNEL_RBF_BROWNIAN:
        assert d == 1
        X = BROWN_X0 + SPACING * P
        head = [BROWN_A[0], 1.0, BROWN_A[1]]
    else:
        ell = np.array(ELL3 if d == 3 else (1.5,))
        X = SPACING * ell * P
        head = [1.0] + list(ell)
    if p is not None:
        q = p // 2 if q is None else q
        assert 0 <= q < p < N
        X[p] = X[q]
    mean_diag = BROWN_A[0] * BROWN_A[1] * float(np.mean(X)) if kid == go.KERNEL_RBF_BROWNIAN else 1.0
    theta = np.array(head + [-shift * mean_diag - go.GPY_DIAG_EPS])
    return X, _targets(N, seed), theta


def rung_of(shift):
    """The ladder's rung (0-based k, jitter = mean(diag Ky) 1e-6 10^k) that rung_window(shift) needs, and that jitter."""
    mean_diag = 1.0 - shift
    for k, r in enumerate(RUNGS):
        if r * mean_diag > shift:
            return k, r * mean_diag
    raise ValueError(shift)


def rung_window(kid, N, d, p, q=None, seed=0, shift=3e-5):
    """The lattice window with the duplicate at p and sigma_n^2 + 1e-8 = -shift: positive definite only from the rung whose
    jitter exceeds `shift`.  Returns X, y, theta, k, jitter (rung_of)."""
    assert kid != go.KERNEL_RBF_BROWNIAN
    X, y, theta = lattice_window(kid, N, d, p, q, seed, shift)
    return (X, y, theta) + rung_of(shift)


def margin(kid, theta, X, jitter=0.0):
    """(info, smallest pivot before the failing one, the failing pivot), pivots in units of mean(diag Ky): the condition of a
    case is info == p + 1, the first >= MARGIN, the second <= -MARGIN."""
    Ky = ky_of(kid, theta, X, jitter)
    info, piv = first_bad_pivot(Ky)
    md = float(np.mean(np.diag(Ky)))
    if info == 0:
        return 0, float(np.min(piv)) / md, None
    return info, (float(np.min(piv[:-1])) / md if info > 1 else np.inf), float(piv[-1]) / md


def ladder_jitters(kid, theta, X):
    """Jitter 0 and the five rungs for this window (mean(diag Ky) * 1e-6 * 10^k)."""
    md = float(np.mean(np.diag(ky_of(kid, theta, X))))
    return [0.0] + [md * r for r in RUNGS]


def lapack_info(Ky, single=False):
    """info of LAPACK's own blocked potrf on the same matrix (dpotrf, or spotrf on the matrix rounded to fp32)."""
    if single:
        return int(sla.lapack.spotrf(np.asarray(Ky, dtype=np.float32), lower=1)[1])
    return int(sla.lapack.dpotrf(np.asarray(Ky, dtype=np.float64), lower=1)[1])


def fit(kid, theta, X, y):
    """The oracle's fit (GPy's ladder included), whichever module knows the kernel; raises go.NotPositiveDefinite."""
    return mo.fit(kid, theta, X, y) if kid in mo.KERNELS else go.fit(kid, theta, X, y)


def predict(f, Xs, include_noise=True):
    return mo.predict(f, Xs, include_noise) if f.kernel_id in mo.KERNELS else go.predict(f, Xs, include_noise)


def lapack_fp32_error(kid, theta, X, y, Xs, f):
    """What plain single-precision LAPACK (spotrf / strtrs on the fp64 Gram matrix rounded to fp32) loses against the fp64
    oracle `f` on variance and logML of this window: the second term of the header's fp32 bar, max(1e-3, 10 x this)."""
    Ky = ky_of(kid, theta, X).astype(np.float32)
    L = sla.cholesky(Ky, lower=True, check_finite=False)
    z = sla.solve_triangular(L, y.astype(np.float32), lower=True, check_finite=False)
    logml = -0.5 * float(z @ z) - float(np.sum(np.log(np.diag(L)))) - 0.5 * len(y) * np.log(2 * np.pi)
    V = sla.solve_triangular(L, go.kernel_K(kid, theta, X, Xs).astype(np.float32), lower=True, check_finite=False)
    var = np.maximum(go.kernel_Kdiag(kid, theta, Xs).astype(np.float32) - np.sum(V * V, 0), 1e-15) + np.float32(theta[-1])
    _, ovar = go.predict(f, Xs)
    return max(abs(logml - f.logml) / abs(f.logml), float(np.max(np.abs(var - ovar) / np.abs(ovar))))


# ---- the cases of tests/test_gpu_failure_paths.py: every GPU case draws its windows from these lists, and
# ---- tests/test_oracle_failure.py walks the same lists, so no window reaches the GPU whose margin was not checked on the CPU
N_TILED, D_TILED, M_TILED = 264, 3, 20       # three block steps 128 + 128 + 8: the last 16-block is partial; M no multiple of 16
# (p, q): first block; a 16-block boundary; the boundary of tiles 0 / 1; the last pivot of tile 1's first 16-block; a 16-block
# boundary inside tile 1; the first pivot of the partial tile; the last row.  q = p // 2 puts the twin in an earlier block or
# tile (the failure arrives through the panel update); the two pairs with q = p - 1 keep both rows of the pair next to each other
# across a tile boundary and inside the last 16-block.
POSITIONS = [(1, 0), (15, 7), (16, 8), (127, 63), (128, 64), (143, 71), (191, 95), (192, 96), (256, 128), (263, 131),
             (128, 127), (263, 262)]
SHORT = [(144, 3), (37, 1)]                  # (N, d) of the one-launch short-window kernels


def short_positions(N):
    return [1, 16, 17, N - 1]


WRAP = 23                                    # ticks pushed beyond N before the "wrapped" window cases
WINDOWS = [(80, 1, 0), (80, 16, 0), (80, 79, 0), (80, 16, WRAP), (200, 130, 0), (200, 130, WRAP)]   # (N, p, start), d = 3
RUNG_SHIFTS = (3e-5, 3e-6, 3e-4)             # rungs k = 2, 1, 3


def hopeless_cases():
    """(kid, N, d, p, q, start) of every window that must fail at p + 1 on every rung."""
    out = []
    for kid in (1, 4):
        out += [(kid, N_TILED, D_TILED, p, q, 0) for p, q in POSITIONS]
    out += [(2, N_TILED, 1, p, q, 0) for p, q in POSITIONS]
    for N, d in SHORT:
        out += [(1, N, d, p, p // 2, 0) for p in short_positions(N)]
    for N in (144, 37):
        out += [(2, N, 1, p, p // 2, 0) for p in short_positions(N)]
    out += [(1, N, 3, p, p // 2, start) for N, p, start in WINDOWS]
    return sorted(set(out))


def rung_cases():
    """(kid, N, d, p, q, shift) of every window that needs exactly one rung."""
    return [(1, N_TILED, D_TILED, 192, 96, s) for s in RUNG_SHIFTS]
