"""Refit oracle of the sliding windows' joint forecast (cgp_window_predict_cov, cgp_window_sample), on top of
oracle/gp_oracle.py: the samples a stream leaves in a window of length N, fitted from scratch, the full posterior covariance at
Xs and sample paths from it.  Test infrastructure (the GPU tests, the fuzz script, the benchmark tool and the C caller's test
compare against it; tests/test_oracle_window_joint.py checks it against forecast_oracle)."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as go


def sliding_window_joint(kernel_id, theta, N, xs, ys, Xs, include_noise=True):
    """Joint forecast at Xs from the window a stream (xs, ys) leaves behind: the last min(len(ys), N) samples refitted from
    scratch; the prior for an empty stream.  Returns (mean (M,), cov (M, M)): cov = K(Xs, Xs) - V^T V with the diagonal
    clipped like go.predict's variance; include_noise adds the noise variance to the diagonal only."""
    Xs = np.asarray(Xs, dtype=np.float64)
    if Xs.ndim == 1:
        Xs = Xs[:, None]
    noise = go.noise_var(kernel_id, theta) if include_noise else 0.0
    cov = go.kernel_K(kernel_id, theta, Xs)
    mean = np.zeros(len(Xs))
    if len(ys) > 0:
        xs = np.asarray(xs, dtype=np.float64).reshape(len(ys), -1)
        f = go.fit(kernel_id, theta, xs[-N:], np.asarray(ys, dtype=np.float64)[-N:])
        Ks = go.kernel_K(kernel_id, theta, f.X, Xs)
        V = sla.solve_triangular(f.L, Ks, lower=True)
        mean = Ks.T @ f.alpha
        cov = cov - V.T @ V
    cov = 0.5 * (cov + cov.T)
    i = np.arange(len(Xs))
    cov[i, i] = np.clip(cov[i, i], go.GPY_VAR_FLOOR, np.inf) + noise
    return mean, cov


def sample_matrix(cov_latent, noise, jitter_rel):
    """The matrix cgp_window_sample factors: cov_latent + noise I + jitter_rel * mean(diag of that sum) I."""
    A = np.array(cov_latent, dtype=np.float64) + noise * np.eye(len(cov_latent))
    return A + jitter_rel * np.mean(np.diag(A)) * np.eye(len(A))


def sample_paths(mean, cov_latent, noise, jitter_rel, xi):
    """Sample paths mean + C xi, C the lower Cholesky factor of sample_matrix(...); xi (S, M) standard normals -> (S, M).
    Raises numpy.linalg.LinAlgError when the matrix is not positive definite (no jitter ladder)."""
    C = np.linalg.cholesky(sample_matrix(cov_latent, noise, jitter_rel))
    xi = np.asarray(xi, dtype=np.float64).reshape(-1, len(mean))
    return np.asarray(mean)[None, :] + xi @ C.T
