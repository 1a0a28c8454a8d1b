"""tests/matern_oracle.py (the float64 reference of the Matern kernels the GPU tests compare against) pinned to sources that
share nothing with it: the scikit-learn, closed-form and 50-digit mpmath fixtures of tests/golden/gen_matern_golden.py, central
differences for its gradient, and a refit for its sliding-window stream.  No GPU."""
import glob
import os

import numpy as np
import pytest

import matern_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "matern_*.npz")))
KIDS = list(mo.KERNELS)


def test_fixture_set_is_complete():
    want = {f"matern_{src}_{tag}_{shape}.npz" for tag in ("m32", "m52") for src, shape in
            (("sk", "n134_d1"), ("sk", "n256_d3"), ("sk", "n2048_d6"), ("closed", "n1"), ("closed", "n2"), ("mp", "n134"))}
    assert want == set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    kid, th = int(z["kernel_id"]), z["theta"]
    tol = 1e-9 if "n2048" in name else 1e-10
    f = mo.fit(kid, th, z["X"], z["y"])
    assert f.jitter == 0.0
    mean, var = mo.predict(f, z["Xs"], include_noise=False)
    scale = max(float(np.max(np.abs(z["mean"]))), 1e-300)
    assert np.max(np.abs(mean - z["mean"])) <= tol * scale
    assert np.max(np.abs(var - z["var_latent"]) / z["var_latent"]) <= tol
    assert abs(f.logml - float(z["logml"])) <= tol * abs(float(z["logml"]))
    assert np.max(np.abs(f.alpha - z["alpha"])) <= tol * np.max(np.abs(z["alpha"]))
    nll, g = mo.nll_and_grad(kid, th, z["X"], z["y"])
    assert nll == -f.logml
    assert np.max(np.abs(-g - z["dlogml_dtheta"])) <= tol * np.max(np.abs(z["dlogml_dtheta"]))
    mean2, cov = mo.predict_cov(f, z["Xs"][:40], include_noise=True)
    assert np.array_equal(cov, cov.T) and np.allclose(np.diag(cov), var[:40] + th[-1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("kid", KIDS)
@pytest.mark.parametrize("d", [1, 3])
def test_gradient_against_central_differences(kid, d):
    rng = np.random.default_rng(10 * kid + d)
    X = rng.uniform(-2, 2, (60, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=60)
    th = np.concatenate([[0.8], rng.uniform(0.6, 2.0, d), [0.05]])
    _, g = mo.nll_and_grad(kid, th, X, y)
    for i in range(len(th)):
        h = 1e-5 * th[i]
        tp, tm = th.copy(), th.copy()
        tp[i] += h
        tm[i] -= h
        fd = (-mo.fit(kid, tp, X, y).logml + mo.fit(kid, tm, X, y).logml) / (2 * h)
        assert abs(g[i] - fd) <= 1e-6 * max(abs(fd), 1.0)


@pytest.mark.parametrize("kid", KIDS)
def test_coincident_points(kid):
    """r = 0: the covariance is sigma_f^2 exactly, dk/dr^2 is finite (-1.5 resp. -5/6 of sigma_f^2), the gradient is finite."""
    th = np.array([1.7, 0.4, 2.0, 0.1])
    X = np.array([[0.25, -1.0], [0.25, -1.0], [1.0, 0.5]])
    K = mo.kernel_K(kid, th, X)
    assert K[0, 1] == th[0] and np.all(np.diag(K) == th[0]) and np.array_equal(mo.kernel_Kdiag(kid, th, X), np.full(3, th[0]))
    k, dk = mo.radial(kid, np.zeros(1))
    assert k[0] == 1.0 and dk[0] == (-1.5 if kid == mo.KERNEL_MATERN32_ARD else -5.0 / 6.0)
    _, g = mo.nll_and_grad(kid, th, X, np.array([0.3, 0.2, -0.5]))
    assert np.all(np.isfinite(g))
    assert np.all(np.isfinite(mo.radial(kid, np.array([-1e-18, 1e-300, 1e300]))[0]))     # clipped, no overflow, no NaN


@pytest.mark.parametrize("kid", KIDS)
def test_sliding_window_stream_against_refit(kid):
    rng = np.random.default_rng(kid)
    T, N, d = 70, 24, 2
    xs = np.column_stack([np.arange(T) / 10.0, rng.normal(size=T)])
    ys = np.sin(xs[:, 0]) + 0.05 * rng.normal(size=T)
    th = np.array([0.9, 1.2, 2.0, 0.01])
    pm, pv, lm, rec = mo.sliding_window_stream(kid, th, N, xs, ys, record_at=(5, 23, 24, 69))
    assert np.array_equal(mo.sliding_window_stream(kid, th, N, xs, ys)[2], lm)
    assert pm[0] == 0.0 and pv[0] == th[0] + th[-1]
    for t in (5, 24, 69):                      # filling, the first tick that drops a sample, the end
        lo = max(0, t + 1 - N)
        assert np.array_equal(rec[t][0], xs[lo:t + 1]) and np.array_equal(rec[t][1], ys[lo:t + 1])
        assert lm[t] == mo.fit(kid, th, xs[lo:t + 1], ys[lo:t + 1]).logml
        lo = t - (N - 1) if t >= N else 0      # the oldest sample leaves before tick t is predicted
        mu, var = mo.predict(mo.fit(kid, th, xs[lo:t], ys[lo:t]), xs[t:t + 1])
        assert pm[t] == mu[0] and pv[t] == var[0]


def test_optimize_improves_and_counts():
    z = np.load(os.path.join(GOLDEN, "matern_mp_m52_n134.npz"))
    th, logml, nev = mo.optimize(4, z["X"], z["y"])
    assert logml > float(z["logml"]) and 5 < nev < 200 and np.all(th > 0)
    assert abs(mo.fit(4, th, z["X"], z["y"]).logml - logml) <= 1e-9 * abs(logml)
