"""CPU tests of the leave-one-out oracle (tests/loo_oracle.py) that the GPU tests of cgp_loo* / cgp_window_loo* compare with:
the closed form against N brute-force refits and against the 50-digit pins of tests/golden/gen_loo_golden.py, and the N = 1 and
N = 2 closed forms.
Bound on closed form against brute force: both are backward-stable Cholesky solves with Ky (or Ky less one row and column), so
each of loo_mean, loo_var (relative) and loo_lpd -- smooth functions of Ky^-1 with sensitivities of order one on these windows --
may differ by a small multiple of cond(Ky) eps; asserted: 16 cond(Ky) eps each, N times that for lpd_sum.  Measured on the shapes
below (the golden windows and the GPU tests' synthetic windows, kernel ids 0-4, d in {1, 3, 6}, N in {130, 257}, cond(Ky) up to
2e4, the RBF x Brownian windows 3e5): <= 9e-14 in the mean, <= 3e-13 relative in the variance, <= 7e-13 in loo_lpd and <= 4e-12
in lpd_sum, five orders under the GPU tests' bar."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
import loo_oracle as lo
import matern_oracle as mo
import corenav_gp_amd.synth as synth


def theta_of(kid, d):   # the GPU tests' thetas (tests/test_gpu_loo.py)
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])


def window(N, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + N, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [rng.normal(size=N) for _ in range(d - 1)]), y


def agree(a, b, Ky):
    e = (np.max(np.abs(a.mean - b.mean)), np.max(np.abs(a.var - b.var) / b.var), np.max(np.abs(a.lpd - b.lpd)),
         abs(a.lpd_sum - b.lpd_sum))
    cond = np.linalg.cond(Ky)
    print("closed form vs brute force: mean %.2e var %.2e lpd %.2e sum %.2e" % e, "cond(Ky) %.2e" % cond)
    bound = 16.0 * cond * np.finfo(np.float64).eps
    assert max(e[:3]) <= bound and e[3] <= len(Ky) * bound and max(e) <= 1e-11, (e, bound)


GOLDEN = ["sk_se_iso_n256_d3", "sk_se_ard_n134_d6", "sk_se_ard_n15_d3", "sk_se_ard_n2_d1", "mp_rbfbrownian_n134",
          "sk_se_ard_n256_d6", "matern_sk_m32_n256_d3", "matern_sk_m52_n256_d3", "matern_mp_m32_n134", "matern_mp_m52_n134"]


@pytest.mark.parametrize("name", GOLDEN)
def test_closed_form_is_brute_force_on_the_golden_windows(name):
    g = load_golden(name)
    X, y, theta, kid = g["X"], g["y"], g["theta"], int(g["kernel_id"])
    a = lo.loo(kid, theta, X, y)
    agree(a, lo.loo_brute(kid, theta, X, y, a.jitter), lo.ky_of(kid, theta, X, a.jitter))
    assert abs(a.logml - float(g["logml"])) <= 1e-9 * abs(float(g["logml"]))


@pytest.mark.parametrize("kid,d", [(0, 1), (0, 3), (1, 3), (1, 6), (2, 1), (3, 1), (3, 6), (4, 3)])
@pytest.mark.parametrize("N", [130, 257])
def test_closed_form_is_brute_force_on_the_synthetic_windows(kid, d, N):
    X, y = window(N, d, 100 * N + d)
    theta = theta_of(kid, d)
    a = lo.loo(kid, theta, X, y)
    assert np.linalg.cond(lo.ky_of(kid, theta, X)) <= 2e4 or kid == 2
    agree(a, lo.loo_brute(kid, theta, X, y, a.jitter), lo.ky_of(kid, theta, X, a.jitter))
    assert a.lpd_sum == float(np.sum(a.lpd))


@pytest.mark.parametrize("src,pin", [("mp_rbfbrownian_n134", "loo_mp_rbfbrownian_n134"), ("matern_mp_m32_n134", "loo_mp_m32_n134"),
                                     ("matern_mp_m52_n134", "loo_mp_m52_n134")])
def test_closed_form_meets_the_mpmath_pins(src, pin):
    """50-digit LU inverse (written from the definitions, nothing shared with the oracle) against the float64 closed form: 1e-9
    in loo_oracle.check's metric, three orders under the GPU bar (cond(Ky) of these windows is <= 1e5)."""
    g, p = load_golden(src), load_golden(pin)
    assert str(p["fixture"]) == src and int(p["kernel_id"]) == int(g["kernel_id"]) and np.array_equal(p["theta"], g["theta"])
    a = lo.loo(int(g["kernel_id"]), g["theta"], g["X"], g["y"])
    assert a.jitter == 0.0
    e = lo.check((a.mean, a.var, a.lpd, a.lpd_sum), lo.Loo(p["loo_mean"], p["loo_var"], p["loo_lpd"], float(p["lpd_sum"]), None, 0.0),
                 g["y"], 1e-9)
    print("oracle vs 50 digits:", e)
    assert abs(float(p["lpd_sum"]) - float(np.sum(p["loo_lpd"]))) <= 1e-12 * abs(float(p["lpd_sum"]))


@pytest.mark.parametrize("kid", [0, 1, 2, 3, 4])
def test_n1_is_the_prior_and_n2_the_two_by_two_inverse(kid):
    d = 1
    theta = theta_of(kid, d)
    noise = float(theta[-1])
    X, y = np.array([[3.0], [5.0]]), np.array([0.7, -0.2])
    kxx = (mo.kernel_Kdiag if kid >= 3 else go.kernel_Kdiag)(kid, theta, X)
    a = lo.loo(kid, theta, X[:1], y[:1])
    c = kxx[0] + noise + 1e-8
    assert abs(a.mean[0]) <= 4e-16 and abs(a.var[0] - c) <= 1e-15 * c   # y - alpha / kd rounds
    assert abs(a.lpd[0] - (-0.5 * np.log(2 * np.pi * c) - 0.5 * y[0] ** 2 / c)) <= 1e-14 and a.lpd_sum == a.lpd[0]
    Ky = lo.ky_of(kid, theta, X)
    (p, b), (_, q) = Ky
    a = lo.loo(kid, theta, X, y)
    wm, wv = np.array([b * y[1] / q, b * y[0] / p]), np.array([p - b * b / q, q - b * b / p])
    assert np.max(np.abs(a.mean - wm)) <= 1e-14 and np.max(np.abs(a.var - wv) / wv) <= 1e-13
    assert np.max(np.abs(a.lpd - lo.lpd_of(y, wm, wv))) <= 1e-12 and a.lpd_sum == float(np.sum(a.lpd))


def test_jitter_ladder_is_inside_the_oracle():
    """test_gpu_loo.py::test_jitter_ladder_is_per_fit's near-singular window: loo runs GPy's ladder, loo_var includes the jitter
    (brute force at the same diagonal agrees; at the diagonal without it the refits are not positive definite)."""
    N = 200
    X = np.repeat(np.arange(N // 2, dtype=float), 2)[:, None]
    y = np.sin(X[:, 0])
    th = np.array([1.0, 3.0, -1e-8 - 2e-7])
    a = lo.loo(0, th, X, y)
    assert a.jitter > 0 and np.all(a.var > 0)
    b = lo.loo_brute(0, th, X, y, a.jitter)
    assert np.max(np.abs(a.var - b.var) / b.var) <= 1e-6 and np.max(np.abs(a.mean - b.mean)) <= 1e-6
    with pytest.raises(np.linalg.LinAlgError):
        lo.loo_brute(0, th, X, y, 0.0)
    with pytest.raises(go.NotPositiveDefinite):
        lo.loo(0, np.array([1.0, 1.0, -2.0]), X, y)
