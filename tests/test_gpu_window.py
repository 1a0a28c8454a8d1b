"""GPU parity of the online sliding-window GP (BASELINE configs[3]: rank-1 Cholesky update per tick)
against the oracle, which refits the current window from scratch at every tick."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu
TOL = 1e-6


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def stream(T, d, seed, tick0=11):
    rng = np.random.default_rng(seed)
    t = np.arange(tick0, tick0 + T, dtype=np.float64)
    y = synth._slip_series(rng, t)
    if d == 1:
        return t[:, None], y
    X = np.column_stack([(t - t.mean()) / t.std()] + [rng.normal(size=T) for _ in range(d - 1)])
    return X, y


@pytest.mark.parametrize("kid,N,d,T", [(2, 16, 1, 60), (2, 40, 1, 130), (0, 33, 2, 100), (1, 64, 3, 200), (1, 100, 6, 260)])
def test_stream_matches_refit_oracle(engine, kid, N, d, T):
    X, y = stream(T, d, 100 + N)
    theta = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3]),
             1: np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])}[kid]
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, kid, theta)
    # fed in three uneven blocks: the state must carry across launches (and across compactions)
    cuts = [0, T // 3, T // 3 + 7, T]
    pm, pv, lm = [np.concatenate(a) for a in zip(*[
        [o[0] for o in ctx.window_push(X[a:b][None], y[a:b][None])] for a, b in zip(cuts[:-1], cuts[1:])])]
    opm, opv, olm = go.sliding_window_stream(kid, theta, N, X, y)
    assert ctx.window_state(0) == (min(N, T), 0)
    assert np.max(np.abs(pm - opm)) <= TOL * max(np.max(np.abs(opm)), 1e-12)
    assert np.max(np.abs(pv - opv) / opv) < TOL
    assert np.max(np.abs(lm - olm) / np.maximum(np.abs(olm), 1.0)) < TOL


def test_config4_window512_checkpoints(engine):
    """configs[3] size: N = 512, compared with a from-scratch refit at a few ticks after the window
    has turned over more than twice (rounding of ~1100 chained rank-1 updates stays far below 1e-6)."""
    N, d, T = 512, 3, 1200
    X, y = stream(T, d, 7)
    theta = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    pm, pv, lm = (o[0] for o in ctx.window_push(X[None], y[None]))
    for t in (N - 1, N, 2 * N + 3, T - 1):
        lo = max(0, t + 1 - N)
        f = go.fit(1, theta, X[lo:t + 1], y[lo:t + 1])
        assert abs(lm[t] - f.logml) <= TOL * abs(f.logml)
        fp = go.fit(1, theta, X[max(0, t - N + 1):t], y[max(0, t - N + 1):t]) if t >= N else go.fit(1, theta, X[:t], y[:t])
        mu, var = go.predict(fp, X[t:t + 1])
        assert abs(pm[t] - mu[0]) <= TOL * max(abs(mu[0]), 1e-3) and abs(pv[t] - var[0]) <= TOL * var[0]


def test_config4_as_written_10000_ticks(engine):
    """BASELINE configs[3] as written: N = 512 ring, 10 000 ticks streamed (one append + one drop per tick, fed
    in blocks of 2 500 so the state also crosses launches), checked against a from-scratch refit of the
    current window at checkpoints up to the last tick: ~9 500 chained rank-1 up/downdates and ~19 ring
    compactions keep the 1e-6 bar."""
    N, d, T = 512, 3, 10000
    X, y = stream(T, d, 11)
    theta = np.array([0.02, 1.0, 1.4, 0.9, 1e-3])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(1, N, d, 1, theta)
    outs = [ctx.window_push(X[a:a + 2500][None], y[a:a + 2500][None]) for a in range(0, T, 2500)]
    pm, pv, lm = (np.concatenate([o[q][0] for o in outs]) for q in range(3))
    assert ctx.window_state(0) == (N, 0)
    assert np.all(np.isfinite(lm)) and np.all(pv > theta[-1] * (1 - 1e-9))
    for t in (N - 1, N, 2499, 2500, 5000, 7777, T - 1):
        lo = max(0, t + 1 - N)
        f = go.fit(1, theta, X[lo:t + 1], y[lo:t + 1])
        assert abs(lm[t] - f.logml) <= TOL * abs(f.logml), t
        fp = go.fit(1, theta, X[max(0, t - N + 1):t], y[max(0, t - N + 1):t]) if t >= N else go.fit(1, theta, X[:t], y[:t])
        mu, var = go.predict(fp, X[t:t + 1])
        assert abs(pm[t] - mu[0]) <= TOL * max(abs(mu[0]), 1e-3) and abs(pv[t] - var[0]) <= TOL * var[0], t


def test_many_windows_independent(engine):
    nwin, N, d, T = 5, 24, 1, 70
    Xs, ys = zip(*[stream(T, d, 300 + w, tick0=11 + 5 * w) for w in range(nwin)])
    theta = np.array([[0.5, 20.0 + w, 0.01, 0.002] for w in range(nwin)])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, 2, theta)
    pm, pv, lm = ctx.window_push(np.stack(Xs), np.stack(ys))
    for w in range(nwin):
        opm, opv, olm = go.sliding_window_stream(2, theta[w], N, Xs[w], ys[w])
        assert np.max(np.abs(pm[w] - opm)) <= TOL * np.max(np.abs(opm))
        assert np.max(np.abs(lm[w] - olm) / np.abs(olm)) < TOL


def test_many_windows_take_the_packed_paired_kernel(engine):
    """A context of >= 1024 windows runs its steady-state ticks two per pass over the factor with TWO windows per workgroup
    (rows of wave 0 split between them): 1024 windows of N = 48 with different data and hyper-parameters each, streamed in
    uneven blocks across ring compactions; a sample of windows -- both members of a workgroup's pair, first / last workgroup
    -- against the refit-per-tick oracle, and every window's status clean."""
    W, N, d, T = 1024, 48, 2, 230
    rng = np.random.default_rng(1024)
    t = np.arange(11, 11 + T, dtype=np.float64)
    X = np.empty((W, T, d))
    X[:, :, 0] = (t - t.mean()) / t.std()
    X[:, :, 1] = rng.normal(size=(W, T))
    y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] * rng.uniform(0.5, 1.5, (W, 1)) + rng.normal(0, 0.03, (W, T))
    theta = np.column_stack([rng.uniform(0.01, 0.04, W), rng.uniform(0.7, 1.5, (W, d)), np.full(W, 1e-3)])
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(W, N, d, 1, theta)
    cuts = [0, 31, 32, 135, T]          # filling, an odd tick, steady-state runs across a compaction
    outs = [ctx.window_push(X[:, a:b], y[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pm, pv, lm = (np.concatenate([o[k] for o in outs], axis=1) for k in range(3))
    for w in (0, 1, 2, 511, 1022, 1023):
        opm, opv, olm = go.sliding_window_stream(1, theta[w], N, X[w], y[w])
        assert np.max(np.abs(pm[w] - opm)) <= TOL * max(np.max(np.abs(opm)), 1e-12)
        assert np.max(np.abs(pv[w] - opv) / opv) < TOL
        assert np.max(np.abs(lm[w] - olm) / np.maximum(np.abs(olm), 1.0)) < TOL
    assert all(ctx.window_state(w) == (N, 0) for w in (0, 1, 777, 1023))


def test_growing_pushes_of_a_fresh_context_under_load(engine):
    """Regression of the two races round 6's sweeps found with fourteen processes on the GPU (never on an idle one): a fresh
    context's first pushes -- one tick, then seven, then seventeen: each longer than the pinned block the previous one left --
    used to come back, about once in a hundred under load, with the outputs of a push untouched (the kernels access that block in
    place; it was freed and allocated again between pushes), and cgp_window_init's asynchronous fill of the windows' state words
    was not ordered before the first push on the context's non-blocking stream (a memory access fault).  Here: the failing case
    of the sweep, 300 fresh contexts, while five other processes keep the GPU busy with fits (six on the GPU with this
    one, never more: the GPU may be shared with other jobs)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    N, d, kid, T, nwin, cuts, seed = 3, 1, 2, 25, 2, [0, 1, 8, 25], 581800996
    X, y = [], []
    for w in range(nwin):
        t = np.arange(11 + w, 11 + w + T, dtype=np.float64)
        X.append(t[:, None]); y.append(synth._slip_series(np.random.default_rng(seed + w), t))
    X, y = np.stack(X), np.stack(y)
    theta = np.array([0.5, 30.0, 0.01, 0.002])
    ref = [go.sliding_window_stream(kid, theta, N, X[w], y[w], include_noise=False) for w in range(nwin)]
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    load = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "fuzz", "fuzz_parity.py"), "25", str(40 + i)], env=env, cwd=root,
                             stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for i in range(5)]
    try:
        bad = 0
        for rep in range(300):
            ctx = engine.Context(max_n=8, max_m=8, max_d=d)
            ctx.window_init(nwin, N, d, kid, theta)
            outs = [ctx.window_push(X[:, a:b], y[:, a:b], include_noise=False) for a, b in zip(cuts[:-1], cuts[1:])]
            pm, pv, lm = [np.concatenate([o[i] for o in outs], axis=1) for i in range(3)]
            for w in range(nwin):
                opm, opv, olm = ref[w]
                if not (np.max(np.abs(pm[w] - opm)) < 1e-9 and np.max(np.abs(lm[w] - olm)) < 1e-6 * np.max(np.abs(olm))
                        and np.max(np.abs(pv[w] - opv)) < 1e-9 and ctx.window_state(w) == (N, 0)):
                    bad += 1
        assert bad == 0, bad
    finally:
        for p in load:
            p.wait(timeout=120)


def test_many_windows_take_four_ticks_per_pass_and_match_single_ticks(engine):
    """From 512 windows the steady-state ticks go four per pass over the factor (k_window_multi; rows born inside the pass, three
    inert lanes in the first panel): the same stream pushed tick by tick (k_window_ticks only) gives the same outputs to rounding,
    and window 0 matches the refit oracle.  Window lengths either side of a panel boundary; block lengths that are no multiple of four; one block
    longer than the ring (the compacting tick goes through the single-tick kernel in the middle of it)."""
    for N, d, T2 in ((64, 2, 23), (81, 3, 38), (64, 1, 150)):   # the last one runs through a ring compaction inside the block
        nwin, kid = 512, 1
        rng = np.random.default_rng(N)
        T = N + 6 + T2
        t = np.arange(11, 11 + T, dtype=np.float64)
        X = np.empty((nwin, T, d)); X[:, :, 0] = (t - t.mean()) / t.std(); X[:, :, 1:] = rng.normal(size=(nwin, T, d - 1))
        y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] + rng.normal(0, 0.03, (nwin, T))
        theta = np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]])
        A = engine.Context(max_n=8, max_m=8, max_d=d); A.window_init(nwin, N, d, kid, theta)
        B = engine.Context(max_n=8, max_m=8, max_d=d); B.window_init(nwin, N, d, kid, theta)
        n0 = N + 6
        A.window_push(X[:, :n0], y[:, :n0]); B.window_push(X[:, :n0], y[:, :n0])
        pa = A.window_push(X[:, n0:], y[:, n0:])                      # one block: four ticks per pass, then the odd ones
        pb = [np.concatenate(c, 1) for c in zip(*[B.window_push(X[:, j:j + 1], y[:, j:j + 1]) for j in range(n0, T)])]
        for a, b in zip(pa, pb):
            # two orders of the same updates: rounding apart, growing with the number of chained ticks (1.8e-9 after 150 on the dense d = 1 window)
            assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)) < (1e-9 if T2 < 64 else 1e-7)
        opm, opv, olm = go.sliding_window_stream(kid, theta, N, X[0], y[0])
        assert np.max(np.abs(pa[0][0] - opm[n0:])) <= TOL * np.max(np.abs(opm))
        assert np.max(np.abs(pa[1][0] - opv[n0:]) / opv[n0:]) < TOL
        assert np.max(np.abs(pa[2][0] - olm[n0:]) / np.maximum(np.abs(olm[n0:]), 1.0)) < TOL
        assert A.window_state(0) == (N, 0) and A.window_state(nwin - 1) == (N, 0)

