"""Refit oracle of the multi-target sliding windows (cgp_window_predict_multi): P target columns on one stream of inputs, each
column "refitted on the current window" -- tests/forecast_oracle.py::sliding_window_forecast per column (the Matern pair, which
oracle/gp_oracle.py does not hold, through tests/matern_oracle.py in the same way), logml from the same refit.  Nothing is
shared between the columns here; tests/test_oracle_window_multi.py checks it against the one-factor restatement
tests/multi_oracle.py::fit_predict_multi.  Test infrastructure."""
import numpy as np

from oracle import gp_oracle as go
import forecast_oracle as fo
import matern_oracle as mo


def _mod(kid):
    return mo if kid in mo.KERNELS else go


def prior(kid, theta, Xs, P, include_noise=True):
    """The empty-window rule: mean 0 (P, M), the prior variance (M,), logml 0 (P,)."""
    Xs = np.asarray(Xs, dtype=np.float64).reshape(len(Xs), -1)
    nv = (mo.noise_var(theta) if kid in mo.KERNELS else go.noise_var(kid, theta)) if include_noise else 0.0
    return np.zeros((P, len(Xs))), _mod(kid).kernel_Kdiag(kid, theta, Xs) + nv, np.zeros(P)


def sliding_window_forecast_multi(kid, theta, N, xs, Ys, Xs, include_noise=True, want_jitter=False):
    """xs (T, d) the stream's inputs, Ys (T, P) its targets, Xs (M, d) -> mean (P, M), var (M,), logml (P,) of the window the
    stream leaves behind (its last min(T, N) samples).  want_jitter: also the largest jitter a column's refit needed (0.0: the
    window is positive definite as it stands, which is what a resident window needs)."""
    Ys = np.asarray(Ys, dtype=np.float64)
    T, P = Ys.shape
    Xs = np.asarray(Xs, dtype=np.float64).reshape(len(Xs), -1)
    if T == 0:
        out = prior(kid, theta, Xs, P, include_noise)
        return out + (0.0,) if want_jitter else out
    xs = np.asarray(xs, dtype=np.float64).reshape(T, -1)
    o = _mod(kid)
    means, vars_, lml, jit = [], [], [], 0.0
    for p in range(P):
        if o is go:
            mu, var = fo.sliding_window_forecast(kid, theta, N, xs, Ys[:, p], Xs, include_noise)
        else:
            mu, var = mo.predict(mo.fit(kid, theta, xs[-N:], Ys[-N:, p]), Xs, include_noise)
        f = o.fit(kid, theta, xs[-N:], Ys[-N:, p])
        means.append(mu)
        vars_.append(var)
        lml.append(f.logml)
        jit = max(jit, f.jitter)
    for v in vars_[1:]:
        assert np.array_equal(v, vars_[0])
    out = (np.stack(means), vars_[0], np.array(lml))
    return out + (jit,) if want_jitter else out


def stream(T, d, P, seed, tick0=11):
    """The stream and theta generators of tests/test_gpu_window_pgrad.py (well-conditioned windows for all five kernel ids) with
    P target columns: slip series of their own on the one time axis, scaled differently.  Returns X (T, d), Y (T, P)."""
    import corenav_gp_amd.synth as synth
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + T, dtype=np.float64)
    Y = np.column_stack([(1.0 + 0.25 * p) * synth._slip_series(np.random.default_rng(seed * 131 + p), t) for p in range(P)])
    if d == 1:
        return t[:, None], Y
    X = np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)])
    return X, Y


def theta_of(kid, d):
    if kid == 2:
        return np.array([0.5, 30.0, 0.01, 0.002])
    if kid == 0:
        return np.array([0.02, 1.0, 1e-3])
    return np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])   # SE-ARD and both Matern


def points_for(kid, X, t, N, M, rng):
    """Test points for the window after t ticks: RBF x Brownian on and off the ticks inside and after the window, else around
    the window's inputs."""
    if kid == 2:
        last, lo = X[max(t, 1) - 1, 0], X[max(t - N, 0), 0]
        after = last + 1.0 + np.arange(M, dtype=np.float64)
        on = np.floor(rng.uniform(lo, last + 1.0, size=M))
        off = on + rng.uniform(0.1, 0.9, size=M)
        pick = rng.integers(0, 3, size=M) if M > 1 else np.array([0])
        return np.where(pick == 0, after, np.where(pick == 1, on, off))[:, None]
    lo = max(0, t - 50)
    return X[rng.integers(lo, max(t, 1), size=M)] + 0.3 * rng.normal(size=(M, X.shape[1]))


def errors(mean, var, logml, omean, ovar, ologml):
    """tests/multi_oracle.py::errors: the mean per column against that column's largest oracle mean, the variance relative,
    logml against max(1, |logml|)."""
    em = np.max(np.max(np.abs(mean - omean), axis=1) / np.maximum(np.max(np.abs(omean), axis=1), 1e-12))
    ev = np.max(np.abs(var - ovar) / ovar)
    el = np.max(np.abs(logml - ologml) / np.maximum(1.0, np.abs(ologml)))
    return em, ev, el
