"""Every kernel path of cgp_window_push, pinned by the launch plan the push itself is cut by (cgp_debug_window_plan), and a window
that loses positive definiteness in mid-stream in each of those kernels beside healthy neighbours.

Every case first asserts the plan of the push it is about to make -- which kernel takes the steady-state ticks, with how many
windows per workgroup or threads per window, and what is left over after the four-tick passes -- so a crossover that moves turns
the case red instead of quietly testing another kernel.  Then a sample of windows is compared with a from-scratch refit of the
current window (oracle/gp_oracle.py, tests/matern_oracle.py) and EVERY window with a second context that is fed the same stream
one tick per push (k_window_ticks only).  Of the matrix's contexts one is alive at a time: the largest holds 9.7 GB of factors."""
import numpy as np
import pytest

from oracle import gp_oracle as go
import matern_oracle as mo

pytestmark = pytest.mark.gpu
TOL = 1e-6
TWIN_TOL = 1e-7   # two orders of the same updates, the bar of test_many_windows_take_four_ticks_per_pass_and_match_single_ticks


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


# ---- oracle of any kernel id ----------------------------------------------------------------------------------------------------
def ofit(kid, theta, X, y):
    return mo.fit(kid, theta, X, y) if kid >= 3 else go.fit(kid, theta, X, y)


def opredict(f, Xs, noise):
    return mo.predict(f, Xs, noise) if f.kernel_id >= 3 else go.predict(f, Xs, noise)


def ostream(kid, theta, N, X, y, noise=True):
    return (mo if kid >= 3 else go).sliding_window_stream(kid, theta, N, X, y, include_noise=noise)


def okernel(kid, theta, X):
    return mo.kernel_K(kid, theta, X) if kid >= 3 else go.kernel_K(kid, theta, X)


def check_tick(kid, theta, N, X, y, t, pm, pv, lm, noise, tag):
    """The outputs of tick t of one window against refits of the window before and after the tick."""
    lo = max(0, t + 1 - N)
    f = ofit(kid, theta, X[lo:t + 1], y[lo:t + 1])
    assert abs(lm[t] - f.logml) <= TOL * max(abs(f.logml), 1.0), (tag, t, lm[t], f.logml)
    mu, var = opredict(ofit(kid, theta, X[max(0, t - N + 1):t], y[max(0, t - N + 1):t]), X[t:t + 1], noise)
    kxx = okernel(kid, theta, X[t:t + 1])[0, 0]
    assert abs(pm[t] - mu[0]) <= TOL * max(abs(mu[0]), 1e-3), (tag, t, pm[t], mu[0])
    assert abs(pv[t] - var[0]) <= TOL * max(var[0], 1e-9 * kxx), (tag, t, pv[t], var[0])


def check_stream(kid, theta, N, X, y, pm, pv, lm, noise, tag):
    opm, opv, olm = ostream(kid, theta, N, X, y, noise)
    kxx = np.array([okernel(kid, theta, X[t:t + 1])[0, 0] for t in range(len(y))])
    assert np.max(np.abs(pm - opm)) <= TOL * max(np.max(np.abs(opm)), 1e-12), tag
    assert np.max(np.abs(pv - opv) / np.maximum(opv, 1e-9 * kxx)) < TOL, tag
    assert np.max(np.abs(lm - olm) / np.maximum(np.abs(olm), 1.0)) < TOL, tag


# ---- streams: data and hyper-parameters of their own for every window -----------------------------------------------------------
def make_streams(kid, nwin, d, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(11, 11 + T, dtype=np.float64)
    if kid == 2:   # RBF x Brownian on the tick time: every window starts at a tick of its own
        X = (t[None, :] + rng.integers(0, 40, (nwin, 1)))[:, :, None]
        theta = np.column_stack([rng.uniform(0.3, 0.7, nwin), rng.uniform(20.0, 40.0, nwin), rng.uniform(0.005, 0.02, nwin),
                                 rng.uniform(1e-3, 4e-3, nwin)])
        amp = np.sqrt((theta[:, 0] * theta[:, 2])[:, None] * X[:, :, 0])
        y = amp * (0.5 * np.sin(2 * np.pi * t / 40.0)[None] * rng.uniform(0.5, 1.5, (nwin, 1)) + rng.normal(0, 0.05, (nwin, T)))
        return X, y, theta
    X = np.empty((nwin, T, d))
    X[:, :, 0] = (t - t.mean()) / t.std() * rng.uniform(0.8, 1.25, (nwin, 1))
    X[:, :, 1:] = rng.normal(size=(nwin, T, d - 1))
    y = 0.1 * np.sin(2 * np.pi * t / 40.0)[None] * rng.uniform(0.5, 1.5, (nwin, 1)) + rng.normal(0, 0.03, (nwin, T))
    # length scales grow with sqrt(d): the windows stay correlated at d = 8 (a diagonal matrix would test nothing)
    ell = rng.uniform(0.7, 1.5, (nwin, 1 if kid == 0 else d)) * np.sqrt(d)
    theta = np.column_stack([rng.uniform(0.01, 0.04, nwin), ell, rng.uniform(0.5e-3, 2e-3, nwin)])
    return X, y, theta


def context(engine, nwin, N, d, kid, theta):
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    ctx.window_init(nwin, N, d, kid, theta)
    return ctx


def assert_covers(plan, T):
    """The launches of a plan are the ticks 0 .. T - 1 in order, each once."""
    t = 0
    for kind, arg, t0, nt in plan:
        assert t0 == t and nt > 0, plan
        assert (kind, arg) in {(0, 256), (0, 512), (1, 1), (1, 2), (2, 4)}, plan
        assert kind == 0 or nt % (2 if kind == 1 else 4) == 0, plan
        t += nt
    assert t == T, (plan, T)


def steady_plan(engine, s, main, wth, wpw_left=1):
    """What a block of s steady-state ticks without a ring compaction is cut into: the main kernel's passes, then what is left
    over -- after four-tick passes a pair and / or a single tick, after pairs a single tick."""
    plan, t = [], 0
    if main[0] == engine.PLAN_MULTI and s >= 4:
        plan.append((engine.PLAN_MULTI, 4, 0, s - s % 4))
        t = s - s % 4
        main = (engine.PLAN_PAIRS, wpw_left)
    if s - t >= 2:
        plan.append((engine.PLAN_PAIRS, main[1], t, (s - t) & ~1))
        t += (s - t) & ~1
    if s - t:
        plan.append((engine.PLAN_TICKS, wth, t, 1))
    return plan


def run_case(engine, kid, nwin, N, d, main, seed, noise=True, wpw_left=1, twin=True, tail=None):
    """One row of the matrix.  The stream: the filling and five steady ticks (one left over), a block that leaves two, one that
    leaves three, and the rest, which runs through the ring compaction at tick 2 N.  main = (kind, windows per workgroup | 4)."""
    P = engine
    wth = 512 if nwin <= 256 else 256
    tail = N + 19 if tail is None else tail
    cuts = [0, N + 5, N + 5 + 14, N + 5 + 14 + 11]
    cuts.append(cuts[-1] + tail)
    T = cuts[-1]
    X, y, theta = make_streams(kid, nwin, d, T, seed)
    tag = f"kid={kid} nwin={nwin} N={N} d={d}"
    ctx = context(engine, nwin, N, d, kid, theta)
    outs, plans = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        plan = ctx.window_plan(b - a)
        assert_covers(plan, b - a)
        plans.append(plan)
        if a == 0:     # the filling is one launch of the single-tick kernel, then the five steady ticks
            assert plan == [(P.PLAN_TICKS, wth, 0, N)] + [(k, g, t0 + N, nt) for k, g, t0, nt in steady_plan(P, 5, main, wth, wpw_left)], (tag, plan)
        elif b < 2 * N:
            assert plan == steady_plan(P, b - a, main, wth, wpw_left), (tag, plan)
        outs.append(ctx.window_push(X[:, a:b], y[:, a:b], include_noise=noise))
    # the last block holds the ring compaction: a single-tick launch in the middle of it, the main kernel on both sides
    last, comp = plans[-1], 2 * N - cuts[-2]
    if T > 2 * N:
        mid = [q for q in last if q[0] == P.PLAN_TICKS and q[2] <= comp < q[2] + q[3]]
        assert len(mid) == 1 and mid[0][1] == wth, (tag, last)
        assert any(q[:2] == main and q[2] + q[3] <= comp for q in last) and any(q[:2] == main and q[2] > comp for q in last), (tag, last)
    else:
        assert any(q[:2] == main for q in last), (tag, last)
    pm, pv, lm = (np.concatenate([o[k] for o in outs], axis=1) for k in range(3))
    assert all(ctx.window_state(w) == (N, 0) for w in (0, nwin // 2, nwin - 1)), tag
    ctx.close()
    assert np.all(np.isfinite(pm)) and np.all(np.isfinite(pv)) and np.all(np.isfinite(lm)), tag
    # a sample of windows against the refit oracle: every tick of a short window, checkpoints of a long one -- first steady tick,
    # either side of launch boundaries, either side of the ring compaction, the last tick
    bounds = sorted({a + q[2] for a, plan in zip(cuts[:-1], plans) for q in plan if a + q[2] > 0})
    marks = {N - 1, N, T - 1} | {b - 1 for b in bounds[:4]} | set(bounds[:4]) | {b - 1 for b in bounds[-2:]} | set(bounds[-2:])
    if T > 2 * N:
        marks |= {2 * N - 1, 2 * N, 2 * N + 1}
    for w in sorted({0, 1, nwin - 2, nwin - 1} & set(range(nwin))):   # both members of the first and of the last workgroup
        if N < 200:
            check_stream(kid, theta[w], N, X[w], y[w], pm[w], pv[w], lm[w], noise, (tag, w))
        else:
            for t in sorted(marks):
                check_tick(kid, theta[w], N, X[w], y[w], t, pm[w], pv[w], lm[w], noise, (tag, w))
    if not twin:
        return
    # every window against the same stream one tick per push: the single-tick kernel only
    ctx = context(engine, nwin, N, d, kid, theta)
    ctx.window_push(X[:, :N], y[:, :N], include_noise=noise)
    ref = []
    for t in range(N, T):
        if t in (N, N + 1, 2 * N, T - 1):
            assert ctx.window_plan(1) == [(P.PLAN_TICKS, wth, 0, 1)], tag
        ref.append(ctx.window_push(X[:, t:t + 1], y[:, t:t + 1], include_noise=noise))
    ctx.close()
    for k, a in enumerate((pm, pv, lm)):
        b = np.concatenate([r[k] for r in ref], axis=1)
        err = np.abs(a[:, N:] - b) / np.maximum(np.abs(b), 1e-3)
        assert np.max(err) < TWIN_TOL, (tag, "output", k, "window", int(np.argmax(np.max(err, axis=1))), float(np.max(err)))


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid,d", [(0, 8), (2, 1), (3, 8)])
def test_a_two_windows_per_workgroup_is_the_main_loop(engine, kid, d):
    """1 024 windows of N = 48: too short for the four-tick kernel, 512 workgroups of two windows each (k_window_pairs<2, false>
    and <2, true>); d = MAXD.  Both members of the first and of the last workgroup against the oracle."""
    run_case(engine, kid, 1024, 48, d, (engine.PLAN_PAIRS, 2), 4800 + kid)


@pytest.mark.parametrize("kid", [1, 4])
def test_b_two_windows_per_workgroup_at_the_largest_lds(engine, kid):
    """N = 544 is just beyond the four-tick kernel's 80 KB of LDS (N <= 542) and still inside the packed pairs' (N <= 546)."""
    for N, steady in ((542, (engine.PLAN_MULTI, 4)), (546, (engine.PLAN_PAIRS, 2)), (547, (engine.PLAN_PAIRS, 1))):
        X, y, theta = make_streams(kid, 1024, 2, N, 1)       # ... which N = 542 still takes; from 547 one window per workgroup again
        c = context(engine, 1024, N, 2, kid, theta)
        c.window_push(X, y)
        assert c.window_plan(8) == [steady + (0, 8)], N
        c.close()
    run_case(engine, kid, 1024, 544, 2, (engine.PLAN_PAIRS, 2), 5440 + kid)


def test_c_one_window_per_workgroup_many_long_windows(engine):
    """512 windows of N = 600 (no multiple of 16): k_window_pairs<1> in 512 workgroups with 62 KB of LDS each."""
    run_case(engine, 1, 512, 600, 3, (engine.PLAN_PAIRS, 1), 6000)


@pytest.mark.parametrize("kid,d", [(0, 3), (2, 1), (3, 3)])
def test_d_four_ticks_per_pass_at_the_benchmark_length(engine, kid, d):
    """512 windows of N = 512, the kernels k_window_multi has never been compared on."""
    run_case(engine, kid, 512, 512, d, (engine.PLAN_MULTI, 4), 5120 + kid)


def test_e_four_ticks_per_pass_odd_length_without_noise(engine):
    run_case(engine, 1, 512, 333, 5, (engine.PLAN_MULTI, 4), 3330, noise=False)


@pytest.mark.parametrize("nwin", [256, 258])
def test_f_either_side_of_the_wide_single_tick_kernel(engine, nwin):
    """256 windows fill and compact with 512 threads per window, 258 with 256; the steady state is k_window_pairs<1> on both sides."""
    run_case(engine, 1, nwin, 200, 7, (engine.PLAN_PAIRS, 1), 2000 + nwin)


@pytest.mark.parametrize("nwin,main,wpw_left", [(511, 1, 1), (512, 2, 1), (1022, 2, 1), (1024, 2, 2), (1025, 2, 1)])
def test_g_one_step_off_each_crossover(engine, nwin, main, wpw_left):
    """N = 64, Matern 5/2: 511 windows go two ticks per pass where 512 go four; what four-tick passes leave over goes to
    k_window_pairs<1> with 511 workgroup pairs (1 022 windows) and with an odd count (1 025), to <2> with 1 024."""
    P = engine
    run_case(engine, 4, nwin, 64, 4, (P.PLAN_PAIRS, 1) if main == 1 else (P.PLAN_MULTI, 4), 6400 + nwin, wpw_left=wpw_left,
             twin=nwin not in (512, 1024))


def test_h_the_longest_window(engine):
    """One window of N = 2 048, the largest cgp_window_init accepts: the filling and forty steady ticks, checkpoints only."""
    run_case(engine, 0, 1, 2048, 1, (engine.PLAN_PAIRS, 1), 2048, twin=False, tail=10)


def test_plan_query_rejects_and_leaves_the_state(engine):
    ctx = engine.Context(max_n=8, max_m=8, max_d=1)
    with pytest.raises(engine.CgpError):
        ctx.window_plan(4)                      # no windows
    ctx.window_init(2, 32, 1, 0, np.array([0.02, 1.0, 1e-3]))
    with pytest.raises(engine.CgpError):
        ctx.window_plan(0)
    assert ctx.window_plan(40, cap=1) == ctx.window_plan(40) == [(0, 512, 0, 32), (1, 1, 32, 8)]
    assert ctx.window_state(0) == (0, 0)


# ---- a window that fails in mid-stream ------------------------------------------------------------------------------------------
def failing_streams(kid, nwin, d, T, seed, victim, tstar):
    """make_streams with a victim: inputs so far apart that its matrix is diagonal to rounding, a noise variance of minus half the
    smallest k(x, x), so that every pivot is about k(x, x) / 2 > 0 -- until tick tstar repeats the input of tick tstar - 1: the
    append pivot is then n (2 k + n) / (k + n) < 0.  Returns X, y, the failing theta and the healthy one."""
    X, y, theta = make_streams(kid, nwin, d, T, seed)
    X[victim] = 0.0
    X[victim, :, 0] = 12.0 * np.arange(1, T + 1)
    X[victim, tstar] = X[victim, tstar - 1]
    y[victim] = np.random.default_rng(seed + 1).normal(0, 0.1, T)
    good = theta.copy()
    if kid == 2:
        good[victim] = [0.5, 1.0, 0.01, 0.002]
    else:
        good[victim, 1:-1] = 1.0
    bad = good.copy()
    kmin = good[victim, 0] * (good[victim, 2] * X[victim, 0, 0] if kid == 2 else 1.0)
    bad[victim, -1] = -0.5 * kmin
    return X, y, bad, good


def assert_numpy_fails_at(kid, theta, N, X, tstar):
    """The construction itself: a plain Cholesky of the victim's window raises at tstar and at no tick before."""
    for t in range(tstar + 1):
        lo = max(0, t + 1 - N)
        K = okernel(kid, theta, X[lo:t + 1]) + (theta[-1] + 1e-8) * np.eye(t + 1 - lo)
        if t < tstar:
            np.linalg.cholesky(K)
        else:
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(K)


def launch_of(plan, t):
    return next(q for q in plan if q[2] <= t < q[2] + q[3])


def run_failure(engine, kid, nwin, N, d, victim, pre, T, tl, expect, seed, revive=False):
    """Two contexts that differ in the victim's theta only: `pre` ticks, then the push under test of T ticks whose tick tl
    (0-based) is the failing one.  expect(plan) asserts which launch tick tl falls into."""
    ts = pre + tl
    K = 6
    X, y, bad, good = failing_streams(kid, nwin, d, pre + T + K, seed, victim, ts)
    assert_numpy_fails_at(kid, bad[victim], N, X[victim], ts)
    A, B = context(engine, nwin, N, d, kid, bad), context(engine, nwin, N, d, kid, good)
    others = np.arange(nwin) != victim
    outs = []
    for c in (A, B):
        o0 = c.window_push(X[:, :pre], y[:, :pre]) if pre else tuple(np.empty((nwin, 0)) for _ in range(3))
        plan = c.window_plan(T)
        assert_covers(plan, T)
        expect(plan)
        *o1, rc = c.window_push(X[:, pre:pre + T], y[:, pre:pre + T], check=False)
        assert rc == (tl + 1 if c is A else 0), rc
        outs.append([np.concatenate([u, v], axis=1) for u, v in zip(o0, o1)])
    states = [A.window_state(w) for w in range(nwin)]
    assert states[victim] == (min(N, pre + T), tl + 1)
    assert all(s == (min(N, pre + T), 0) for w, s in enumerate(states) if w != victim)
    # the victim up to the failing tick against the oracle; everybody else bitwise what they are beside a healthy neighbour
    if ts > 1:
        check_stream(kid, bad[victim], N, X[victim, :ts], y[victim, :ts], *[o[victim, :ts] for o in outs[0]], True, "victim")
    for a, b in zip(*outs):
        assert np.array_equal(a[others], b[others])
    # later calls: the push returns the first failure's code again, the forecast returns it with NaN for the victim
    M = 5
    Xs = X[:, pre + T - M:pre + T] + 0.25
    mean, var, code = A.window_predict(Xs, check=False)
    mb, vb = B.window_predict(Xs)
    assert code == tl + 1 and np.all(np.isnan(mean[victim])) and np.all(np.isnan(var[victim]))
    assert np.array_equal(mean[others], mb[others]) and np.array_equal(var[others], vb[others])
    if revive:   # set_theta on the victim alone brings it back: its resident samples are a valid window under the healthy theta
        logml, info = A.window_set_theta(good, select=~others)
        assert np.all(info == 0) and A.window_state(victim) == (N, 0)
        lo = pre + T - N
        f = ofit(kid, good[victim], X[victim, lo:pre + T], y[victim, lo:pre + T])
        assert abs(logml[victim] - f.logml) <= TOL * abs(f.logml)
        oa, ob = A.window_push(X[:, pre + T:], y[:, pre + T:]), B.window_push(X[:, pre + T:], y[:, pre + T:])
        for u, v in zip(oa, ob):
            assert np.array_equal(u[others], v[others])
            assert np.max(np.abs(u[victim] - v[victim]) / np.maximum(np.abs(v[victim]), 1e-3)) < TOL
    else:
        *oa, rc = A.window_push(X[:, pre + T:], y[:, pre + T:], check=False)
        assert rc == tl + 1    # the tick index of the push that failed, not one of this push
        with pytest.raises(engine.CgpError):
            A.window_push(X[:, pre + T:pre + T + 1], y[:, pre + T:pre + T + 1])
        ob = B.window_push(X[:, pre + T:], y[:, pre + T:])
        for u, v in zip(oa, ob):
            assert np.array_equal(u[others], v[others])
    A.close(); B.close()


@pytest.mark.parametrize("pos,kid,d", [(0, 1, 2), (1, 1, 2), (2, 1, 2), (3, 1, 2), (2, 2, 1), (1, 4, 3)])
def test_failure_inside_a_four_tick_pass(engine, pos, kid, d):
    """512 windows of N = 64: the failing tick at each of the four positions of the second pass of k_window_multi<4> (the rows
    born inside the pass carry their own status), RBF x Brownian and Matern once each; set_theta revives the window."""
    P = engine
    def expect(plan):
        assert launch_of(plan, 4 + pos) == (P.PLAN_MULTI, 4, 0, 20) and plan[1:] == [(P.PLAN_PAIRS, 1, 20, 2), (P.PLAN_TICKS, 256, 22, 1)], plan
    run_failure(engine, kid, 512, 64, d, 200 + pos, 64 + 7, 23, 4 + pos, expect, 700 + pos, revive=True)


@pytest.mark.parametrize("tick", [0, 1])
@pytest.mark.parametrize("member", [0, 1])
@pytest.mark.parametrize("group,kid", [(0, 1), (511, 3)])
def test_failure_in_a_workgroup_of_two_windows(engine, tick, member, group, kid):
    """1 024 windows of N = 48, two per workgroup: first and second tick of a pair (the first is handed from wave 0 to the
    window's tail thread through LDS), the victim first and second member, in the first and the last workgroup (Matern there)."""
    P = engine
    def expect(plan):
        assert plan == [(P.PLAN_PAIRS, 2, 0, 12), (P.PLAN_TICKS, 256, 12, 1)], plan
    run_failure(engine, kid, 1024, 48, 2, 2 * group + member, 48 + 3, 13, 6 + tick, expect, 900 + 4 * tick + 2 * member + (group > 0))


@pytest.mark.parametrize("nwin", [3, 300])
def test_failure_while_filling_and_at_the_compacting_tick(engine, nwin):
    """The single-tick kernel with 512 and with 256 threads per window: a failing row in the middle of a panel while the window
    fills, and the tick that moves the ring back to the origin."""
    P, N, wth = engine, 48, 512 if nwin <= 256 else 256
    def filling(plan):
        assert plan == [(P.PLAN_TICKS, wth, 0, 40)], plan
    run_failure(engine, 0, nwin, N, 1, 1, 0, 40, 21, filling, 300 + nwin)
    def compacting(plan):
        assert plan[:3] == [(P.PLAN_PAIRS, 1, 0, 2), (P.PLAN_TICKS, wth, 2, 1), (P.PLAN_PAIRS, 1, 3, 4)], plan
    run_failure(engine, 0, nwin, N, 1, nwin - 1, 2 * N - 2, 8, 2, compacting, 310 + nwin)


@pytest.mark.parametrize("tick", [0, 1])
def test_failure_code_is_the_same_in_place_by_copy_and_polled(engine, tick):
    """Three windows of N = 32: the push is small enough (<= 16 KB staged) to be read and written in place by the kernels, whose
    copies of the status words the host then reads; the same ticks at the head of a push that is staged by copy return the same
    code from the state words; and as a push of its own the failing tick returns 1 through the polled words."""
    P, nwin, N, d, kid, victim, pre = engine, 3, 32, 1, 0, 1, 32 + 3
    tl = 2 + tick
    for T, inplace in ((6, True), (140, False)):
        assert (nwin * T * (d + 4) * 8 + nwin * 16 <= 16 * 1024) == inplace
        def expect(plan):
            assert launch_of(plan, tl)[:3] == (P.PLAN_PAIRS, 1, 0), plan
        run_failure(engine, kid, nwin, N, d, victim, pre, T, tl, expect, 3200 + tick)
    def single(plan):
        assert plan == [(P.PLAN_TICKS, 512, 0, 1)], plan
    run_failure(engine, kid, nwin, N, d, victim, pre + tl, 1, 0, single, 3200 + tick)


# ---- lifetimes of the windows' four reservations --------------------------------------------------------------------------------
EINVAL, ESTATE = -1, -4   # include/corenav_gp.h


def test_reservation_lifetimes_across_init_and_reserve(engine):
    """The lifetime rules of the windows' reservations, walked in one context: a new cgp_window_init drops all four (multi-target,
    its objective, joint forecast, leave-one-out objective), a new cgp_window_multi_reserve drops the multi-target objective's
    scratch with it and nothing else, and what is reserved afterwards holds nothing of what was dropped.  Two windows of
    capacity 33 (two blocks of 16 and a one-row tail), d = 1, SE kernel, P = 2, joint max_m = 4.  A family is probed at the
    argument-check level: with its reservation a call with a bad argument answers CGP_EINVAL, without it CGP_ESTATE (the state
    is checked first)."""
    W, N, d, kid, P, M, T = 2, 33, 1, 0, 2, 4, 5
    rng = np.random.default_rng(33)
    theta = np.tile([0.9, 1.3, 0.05], (W, 1))
    X = np.cumsum(rng.uniform(0.2, 0.6, (W, T, d)), axis=1)
    Y = np.sin(X) + 0.1 * rng.normal(size=(W, T, P))
    Xs = X[:, -1:, :] + 0.3 * np.arange(1, M + 1)[None, :, None]
    buf = np.zeros(64)
    p, a = engine._p(buf), buf.ctypes.data

    def reserve_all(c):
        assert c.window_multi_reserve(P) == 0 and c.window_multi_grad_reserve() == 0
        assert c.window_joint_reserve(M) == 0 and c.window_loo_grad_reserve() == 0

    def families(c):
        lib, h = c.lib, c.h
        return {"multi": (lib.cgp_window_predict_multi(h, 0, P, p, 1, p, p, p), lib.cgp_window_push_multi(h, 0, P, p, p, 1, p, p, p)),
                "multi_grad": (lib.cgp_window_multi_nll_grad(h, P, None, p, 4, p), lib.cgp_window_multi_nll_grad_device(h, P, None, a, 4, a, None),
                               lib.cgp_window_optimize_multi(h, P, 10, None, p, 2, None, None)),
                "joint": (lib.cgp_window_predict_cov(h, 0, p, 1, p, p), lib.cgp_window_sample(h, 0, p, 1, p, 1, 1e-6, p, None)),
                "loo_grad": (lib.cgp_window_loo_nll_grad(h, None, p, 4, p), lib.cgp_window_loo_nll_grad_device(h, None, a, 4, a, None),
                             lib.cgp_window_optimize_loo(h, 10, None, p, 2, None, None))}

    def held(c):
        out = {}
        for name, codes in families(c).items():
            assert all(rc == codes[0] for rc in codes) and codes[0] in (EINVAL, ESTATE), (name, codes)
            out[name] = codes[0] == EINVAL
        return out

    def one_round(c):
        out = list(c.window_push_multi(X, Y)) + list(c.window_multi_nll_grad()) + list(c.window_loo_nll_grad())
        return out + list(c.window_predict_cov(Xs))

    every, none = dict(multi=True, multi_grad=True, joint=True, loo_grad=True), dict(multi=False, multi_grad=False, joint=False, loo_grad=False)
    ctx = engine.Context(max_n=8, max_m=8, max_d=d)
    assert held(ctx) == none   # no windows
    ctx.window_init(W, N, d, kid, theta)
    assert held(ctx) == none
    reserve_all(ctx)
    assert held(ctx) == every
    # the multi-target reservation made again (windows still empty): its objective's scratch goes with it, the other two stay
    assert ctx.window_multi_reserve(P) == 0
    assert held(ctx) == dict(every, multi_grad=False)
    assert ctx.window_multi_grad_reserve() == 0 and held(ctx) == every
    # the joint and the leave-one-out reservations made again: each goes alone
    assert ctx.window_joint_reserve(M) == 0 and ctx.window_loo_grad_reserve() == 0 and held(ctx) == every
    # new windows: every reservation goes
    ctx.window_init(W, N, d, kid, theta)
    assert held(ctx) == none
    reserve_all(ctx)
    assert held(ctx) == every
    got = one_round(ctx)
    fresh = engine.Context(max_n=8, max_m=8, max_d=d)
    fresh.window_init(W, N, d, kid, theta)
    reserve_all(fresh)
    want = one_round(fresh)
    assert len(got) == len(want) == 11
    for u, v in zip(got, want):
        assert np.all(np.isfinite(u)) and np.array_equal(u, v)
    ctx.close()
    fresh.close()
