"""CPU half of the failure-path tests: every window tests/test_gpu_failure_paths.py hands to the engine (the lists of
tests/failure_oracle.py) fails where it is meant to fail, BY A MARGIN -- a condition on the inputs, established before anything
reaches a GPU.  In the reference factorisation (plain unblocked Cholesky in numpy.longdouble of the oracle's Gram matrix plus
the diagonal addend) every pivot before the failing one is >= 1e-3 mean(diag), the failing one is <= -1e-3 mean(diag), at jitter
0 and at each of the five rungs of GPy's ladder; LAPACK's blocked dpotrf (and spotrf on the matrix rounded to fp32, for the
kernels an fp32 context takes) reports the same index; the oracle's fit gives up on the hopeless windows and stops at the
expected rung on the rung windows."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import failure_oracle as fo


def ids(c):
    return "-".join(str(v) for v in c)


def test_first_bad_pivot_on_known_matrices():
    """The reference itself: a 3 x 3 matrix worked by hand, an identity, and agreement with dpotrf where that succeeds."""
    A = np.array([[4.0, 2.0, 2.0], [2.0, 1.0, 3.0], [2.0, 3.0, 9.0]])       # second pivot 1 - 2^2 / 4 = 0: not positive
    info, piv = fo.first_bad_pivot(A)
    assert info == 2 and list(piv) == [4.0, 0.0]
    A[1, 1] = 2.0                                                            # pivots 4, 1, 9 - 1 - 2^2 / 1 = 4
    info, piv = fo.first_bad_pivot(A)
    assert info == 0 and np.allclose(piv, [4.0, 1.0, 4.0], rtol=1e-15)
    assert fo.first_bad_pivot(np.eye(5))[0] == 0 and fo.first_bad_pivot(-np.eye(5))[0] == 1
    rng = np.random.default_rng(0)
    G = rng.normal(size=(40, 40))
    S = G @ G.T + 0.1 * np.eye(40)
    info, piv = fo.first_bad_pivot(S)
    L = np.linalg.cholesky(S)
    assert info == 0 and np.allclose(piv, np.diag(L) ** 2, rtol=1e-10)


@pytest.mark.parametrize("case", fo.hopeless_cases(), ids=ids)
def test_hopeless_window_fails_at_the_chosen_pivot_with_margin(case):
    kid, N, d, p, q, start = case
    X, y, theta = fo.lattice_window(kid, N, d, p, q, start=start)
    assert np.array_equal(X[p], X[q])
    if d == 3:        # the shape of the fp32 cases: scaled coordinates <= 24 keep the inner-product form of the exponent (2e-4 in fp32) far inside the margin
        assert np.max(np.abs(X / theta[1:1 + d])) <= 24.0
    jitters = fo.ladder_jitters(kid, theta, X)
    assert len(jitters) == 6 and jitters[-1] < fo.SHIFT * np.mean(np.diag(fo.ky_of(kid, theta, X)))   # the last rung does not reach the shift
    for j in jitters:
        info, before, bad = fo.margin(kid, theta, X, j)
        assert info == p + 1, (j, info)
        assert before >= fo.MARGIN and bad <= -fo.MARGIN, (j, before, bad)
        Ky = fo.ky_of(kid, theta, X, j)
        assert fo.lapack_info(Ky) == p + 1
        if kid == 1:                                 # the kernels of the fp32 cases
            assert fo.lapack_info(Ky, single=True) == p + 1
    with pytest.raises(go.NotPositiveDefinite):
        fo.fit(kid, theta, X, y)


@pytest.mark.parametrize("kid,N,d", [(1, fo.N_TILED, 3), (4, fo.N_TILED, 3), (2, fo.N_TILED, 1), (1, 144, 3), (1, 37, 1), (2, 144, 1),
                                     (2, 37, 1), (1, 80, 3), (1, 200, 3)])
def test_lattice_without_a_duplicate_factors_with_margin(kid, N, d):
    """The same lattice and the same negative noise WITHOUT the duplicated row: positive definite, every pivot far from zero --
    the failure of the cases above is the pair's, not the lattice's."""
    X, y, theta = fo.lattice_window(kid, N, d)
    info, smallest, _ = fo.margin(kid, theta, X)
    assert info == 0 and smallest >= 0.7
    assert fo.fit(kid, theta, X, y).jitter == 0.0


@pytest.mark.parametrize("case", fo.rung_cases(), ids=ids)
def test_rung_window_needs_exactly_its_rung(case):
    kid, N, d, p, q, shift = case
    X, y, theta, k, jitter = fo.rung_window(kid, N, d, p, q, shift=shift)
    jitters = fo.ladder_jitters(kid, theta, X)
    assert jitters[k + 1] == pytest.approx(jitter, rel=1e-12)
    for i, j in enumerate(jitters):
        info, before, bad = fo.margin(kid, theta, X, j)
        Ky = fo.ky_of(kid, theta, X, j)
        if i <= k:                                   # jitter 0 and the rungs below k: the pair's pivot is (j - shift)(2 + j - shift) < 0
            assert info == p + 1 and before >= fo.MARGIN and fo.lapack_info(Ky) == p + 1
            assert bad <= -0.5 * (shift - j), (j, bad)          # negative by the gap itself: 1e-13 of fp64 rounding cannot move it
        else:
            assert info == 0 and before >= 0.5 * (j - shift) and fo.lapack_info(Ky) == 0
    f = go.fit(kid, theta, X, y)
    assert f.jitter == pytest.approx(jitter, rel=1e-12) and f.jitter == pytest.approx(fo.RUNGS[k] * (1.0 - shift), rel=1e-12)


def test_every_gpu_position_is_in_the_lists():
    """The positions the issue names, spelled out once: a list that lost one would silently drop its GPU case."""
    assert {p for p, _ in fo.POSITIONS} == {1, 15, 16, 127, 128, 143, 191, 192, 256, 263} and len(fo.POSITIONS) == 12
    assert all(q < p for p, q in fo.POSITIONS)
    assert fo.short_positions(144) == [1, 16, 17, 143] and fo.short_positions(37) == [1, 16, 17, 36]
    assert [k for k, _ in map(fo.rung_of, fo.RUNG_SHIFTS)] == [2, 1, 3]
    assert -(-fo.N_TILED // 128) == 3 and fo.N_TILED % 16 == 8 and fo.M_TILED % 16 != 0
