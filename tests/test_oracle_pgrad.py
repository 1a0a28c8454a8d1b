"""The oracle of the predictive gradients (tests/pgrad_oracle.py) against something it does not share code with:
  * central differences of the oracle's own mean and UNCLIPPED variance, all five kernel ids (id 2: ties |x*| = |x_i| excluded,
    points inside the window off the ticks and the reference's grid after it included).  Step h = 1e-5 in the inputs' units:
    truncation h^2 f''' / 6 and rounding eps |f| / h are both below 1e-6 of the gradients' scale for these windows; the bar is
    2e-6 of the largest gradient entry.
  * a 50-digit mpmath restatement on the N = 134 slipVal window for ids 2, 3 and 4 (tests/golden/pgrad_mp_*_n134.npz, written
    by tests/golden/gen_pgrad_golden.py: every formula from its definition, Ky^-1 by LU, nothing shared with the oracle): 1e-9
    of the largest gradient entry -- Ky's condition number on this window is below 1e6, so fp64 leaves about 1e-10.
  * the tie convention of id 2: at |x*| = |x_i| the bracket is 0, i.e. the gradient is the one-sided derivative from the side
    where |x*| is the larger, and sign(0) = 0."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
import pgrad_oracle as po
import corenav_gp_amd.synth as synth


def theta_of(kid, d):
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
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=N) for _ in range(d - 1)]), y


def points(kid, X, M, rng):
    if kid == 2:   # after the window on the ticks, and inside it off the ticks
        after = X[-1, 0] + 1.0 + np.arange(M // 2, dtype=np.float64)
        inside = X[rng.integers(0, len(X) - 1, size=M - M // 2), 0] + rng.uniform(0.2, 0.8, size=M - M // 2)
        return np.concatenate([after, inside])[:, None]
    return X[rng.integers(0, len(X), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


@pytest.mark.parametrize("kid,N,d", [(0, 60, 3), (1, 80, 6), (2, 134, 1), (3, 70, 2), (4, 90, 4), (3, 50, 1), (4, 50, 8)])
def test_oracle_against_central_differences(kid, N, d):
    rng = np.random.default_rng(100 * kid + N)
    X, y = window(N, d, seed=kid + N)
    theta = theta_of(kid, d)
    Xs = points(kid, X, 12, rng)
    f = po.fit(kid, theta, X, y)
    dmean, dvar = po.predictive_gradients(f, Xs)
    assert dmean.shape == dvar.shape == (12, d)
    h = 1e-5
    fm, fv = np.empty_like(dmean), np.empty_like(dvar)
    for q in range(d):
        e = np.zeros(d)
        e[q] = h
        mp, vp = po.unclipped_mean_var(f, Xs + e)
        mm, vm = po.unclipped_mean_var(f, Xs - e)
        fm[:, q], fv[:, q] = (mp - mm) / (2 * h), (vp - vm) / (2 * h)
    em = np.max(np.abs(dmean - fm)) / np.max(np.abs(dmean))
    ev = np.max(np.abs(dvar - fv)) / np.max(np.abs(dvar))
    print(f"kid {kid}: dmean {em:.3g} dvar {ev:.3g}")
    assert em < 2e-6 and ev < 2e-6, (em, ev)


@pytest.mark.parametrize("tag", ["rbfbrownian", "m32", "m52"])
def test_oracle_against_the_50_digit_restatement(tag):
    z = load_golden(f"pgrad_mp_{tag}_n134")
    kid, th = int(z["kernel_id"]), z["theta"]
    f = po.fit(kid, th, z["X"], z["y"])
    assert f.jitter == 0.0 and len(z["y"]) == 134
    dmean, dvar = po.predictive_gradients(f, z["Xs"])
    mean, var = po.unclipped_mean_var(f, z["Xs"])
    em = np.max(np.abs(dmean - z["dmean"])) / np.max(np.abs(z["dmean"]))
    ev = np.max(np.abs(dvar - z["dvar"])) / np.max(np.abs(z["dvar"]))
    print(f"{tag}: dmean {em:.3g} dvar {ev:.3g}")
    assert em <= 1e-9 and ev <= 1e-9, (em, ev)
    assert np.max(np.abs(mean - z["mean"])) <= 1e-9 * np.max(np.abs(z["mean"]))
    assert np.max(np.abs(var - z["var_latent"])) <= 1e-9 * np.max(np.abs(z["var_latent"]))


def test_brownian_tie_convention():
    """On a sample's tick the derivative of min(|x*|, |x_i|) jumps: the oracle takes the side where |x*| is the larger (bracket
    0), so at a tie it equals the limit of the gradient from just beyond the tick; sign(0) = 0 kills both terms at the origin."""
    X, y = window(40, 1, seed=3)
    theta = theta_of(2, 1)
    f = po.fit(2, theta, X, y)
    tie = X[[5, 20, 33]]
    dk_tie, dkss = po.dK_dxs(2, theta, X, tie)
    dk_above, _ = po.dK_dxs(2, theta, X, tie + 1e-9)
    dk_below, _ = po.dK_dxs(2, theta, X, tie - 1e-9)
    for j, i in enumerate((5, 20, 33)):
        assert abs(dk_tie[i, j, 0] - dk_above[i, j, 0]) < 1e-9 * theta[0] * theta[2]
        assert abs(dk_tie[i, j, 0] - dk_below[i, j, 0]) > 0.5 * theta[0] * theta[2]    # the other side carries R sigma_b^2
    np.testing.assert_array_equal(dkss[:, 0], theta[0] * theta[2])
    dk0, dkss0 = po.dK_dxs(2, theta, X, np.zeros((1, 1)))
    assert np.all(dk0 == 0.0) and dkss0[0, 0] == 0.0
    # negative inputs mirror: the gradient is odd in the pair (x*, x_i)
    dkn, dkssn = po.dK_dxs(2, theta, -X, -(tie + 0.3))
    dkp, dkssp = po.dK_dxs(2, theta, X, tie + 0.3)
    np.testing.assert_allclose(dkn, -dkp, rtol=1e-14)
    np.testing.assert_array_equal(dkssn, -dkssp)
    dmean, dvar = po.predictive_gradients(f, tie)
    assert np.all(np.isfinite(dmean)) and np.all(np.isfinite(dvar))
