"""Oracle of the multi-target fits (cgp_fit_predict_multi_batch): GPy.models.GPRegression(X, Y, kernel) with Y (N, P) is P
independent outputs sharing inputs, kernel and hyper-parameters -- so the oracle is one refit per column, nothing shared."""
import numpy as np

from oracle import gp_oracle as go
import matern_oracle as mo


def fit_predict_multi(kid, theta, X, Y, Xs, noise=True):
    """X (N, d), Y (P, N), Xs (M, d) -> mean (P, M), var (M,), logml (P,): one oracle fit / predict per column (GPy's jitter
    ladder included).  The P variances are one vector: asserted."""
    o = mo if kid >= 3 else go
    means, vars_, lml = [], [], []
    for y in np.asarray(Y, dtype=np.float64):
        f = o.fit(kid, theta, X, y)
        mu, var = o.predict(f, Xs, noise)
        means.append(mu)
        vars_.append(var)
        lml.append(f.logml)
    for v in vars_[1:]:
        assert np.array_equal(v, vars_[0])
    return np.stack(means), vars_[0], np.array(lml)


def errors(mean, var, logml, omean, ovar, ologml):
    """The metric of the multi-target tests: the mean per column against that column's largest oracle mean
    (test_gpu_joint_batch.py::close), the variance relative, logml against max(1, |logml|)."""
    em = np.max(np.max(np.abs(mean - omean), axis=1) / np.maximum(np.max(np.abs(omean), axis=1), 1e-12))
    ev = np.max(np.abs(var - ovar) / ovar)
    el = np.max(np.abs(logml - ologml) / np.maximum(1.0, np.abs(ologml)))
    return em, ev, el
