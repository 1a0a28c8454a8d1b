"""joint_oracle (the refit oracle of cgp_window_predict_cov / cgp_window_sample) against forecast_oracle, against a closed form,
and its sample paths against the covariance they are drawn from."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as go
from forecast_oracle import sliding_window_forecast
from joint_oracle import sliding_window_joint, sample_matrix, sample_paths
import corenav_gp_amd.synth as synth


def stream(T, d, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + T, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    return np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)]), y


@pytest.mark.parametrize("kid,N,d,theta", [(2, 12, 1, [0.5, 30.0, 0.01, 0.002]), (0, 9, 2, [0.02, 1.0, 1e-3]),
                                           (1, 20, 3, [0.02, 0.8, 1.2, 1.6, 1e-3])])
@pytest.mark.parametrize("noise", [True, False])
def test_joint_diagonal_and_mean_are_the_marginal_forecast(kid, N, d, theta, noise):
    T = 2 * N + 3
    X, y = stream(T, d, 10 * N + d)
    theta = np.array(theta)
    rng = np.random.default_rng(N)
    Xs = X[-1:, :] + 1.0 + np.arange(23.0)[:, None] if kid == 2 else X[rng.integers(T - N, T, size=23)] + 0.3 * rng.normal(size=(23, d))
    for t in (0, 5, T):
        mean, cov = sliding_window_joint(kid, theta, N, X[:t], y[:t], Xs, include_noise=noise)
        mu, var = sliding_window_forecast(kid, theta, N, X[:t], y[:t], Xs, include_noise=noise)
        assert np.array_equal(mean, mu) and np.array_equal(cov, cov.T)
        np.testing.assert_allclose(np.diag(cov), var, rtol=1e-9)
        latent = sliding_window_joint(kid, theta, N, X[:t], y[:t], Xs, include_noise=False)[1]
        off = cov - latent
        np.testing.assert_allclose(off, (go.noise_var(kid, theta) if noise else 0.0) * np.eye(len(Xs)), atol=1e-15)


def test_joint_oracle_against_the_closed_form_of_a_two_sample_window():
    g = load_golden("closed_joint_n2_se")
    mean, cov = sliding_window_joint(int(g["kernel_id"]), g["theta"], 2, g["X"], g["y"], g["Xs"], include_noise=False)
    np.testing.assert_allclose(mean, g["mean"], rtol=1e-11)
    np.testing.assert_allclose(cov, g["cov_latent"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(sample_paths(mean, cov, float(g["noise"]), float(g["jitter_rel"]), g["xi"]), g["paths"], rtol=1e-9)


def test_empirical_covariance_of_sample_paths():
    """20 000 paths: their empirical mean and covariance are those they were drawn from, within sampling error."""
    N, d, M, S = 30, 2, 12, 20000
    X, y = stream(50, d, 4)
    theta = np.array([0.02, 1.0, 1e-3])
    rng = np.random.default_rng(8)
    Xs = X[rng.integers(20, 50, size=M)] + 0.5 * rng.normal(size=(M, d))
    mean, cov = sliding_window_joint(0, theta, N, X, y, Xs, include_noise=False)
    A = sample_matrix(cov, 1e-3, 1e-6)
    paths = sample_paths(mean, cov, 1e-3, 1e-6, rng.normal(size=(S, M)))
    assert paths.shape == (S, M)
    sd = np.sqrt(np.diag(A))
    assert np.max(np.abs(paths.mean(0) - mean) / sd) < 5.0 / np.sqrt(S)
    emp = np.cov(paths.T)
    assert np.max(np.abs(emp - A) / np.outer(sd, sd)) < 5.0 * np.sqrt(2.0 / S)


def test_sample_paths_refuses_a_singular_matrix_without_jitter():
    cov = np.ones((3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        sample_paths(np.zeros(3), cov - 1e-3 * np.eye(3), 0.0, 0.0, np.zeros((1, 3)))
    assert np.all(np.isfinite(sample_paths(np.zeros(3), cov, 0.0, 1e-6, np.ones((2, 3)))))
