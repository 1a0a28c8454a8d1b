"""The failure path of every factorisation schedule: WHICH pivot is reported, and what a failed fit does to its neighbours.

include/corenav_gp.h: a positive return or `info` is "a LAPACK-style info = 1-based index of the first non-positive pivot"; the
`*_device` entry points tell the caller to "read dinfo and re-submit the failed fits"; a failed fit "leaves its neighbours
unaffected".  The windows of tests/failure_oracle.py fail at a CHOSEN 0-based row p by a margin no rounding can move
(tests/test_oracle_failure.py establishes it for every window used here, on the CPU), so the assertions below are equalities:
info == p + 1, the healthy fits of a call BITWISE those of a control call without the failure, no status left over in the next
call.  Shape: N = 264 = 128 + 128 + 8 (three block steps, the last 16-block partial), d = 3, M = 20; positions in the first
block, on a 16-block boundary, on the tile boundary, inside tile 1, at the first pivot of the partial tile and in the last row.

Which schedule a call of B fits takes at three block steps, from sched_plan of csrc/cgp_sched_plan.hpp as its constants stand:
    latency     B <= lat_fits_by_steps(fp64, 3) = 28 (fp64) / 24 (fp32)      k_tile_sk / k_trmm_sk: potf2_tile, the pivot merged through *flag
    mid-size    B <= mid_fits(3) = MID_FITS_F64 = 48 / MID_FITS_F32 = 96     k_diag_lean for tile 0, tiles 1 and 2 inside k_panel (diag_next) from pre-update
                                                                             images; fp32 factors the diagonal tile in the fat form here (potf2_tile)
    throughput  beyond, fp64 below FUSED64_BELOW = 512                       the same launches without the images; fp32: the packed form (diag_factor_packed)
    full batch  fp64 B >= FUSED64_BELOW = 512                                a k_diag_lean launch of its own per block step, k_panel without a diagonal tile
A single fit (cgp_fit, the ladder's retries, cgp_nll_grad's gradient-mode factorisation) is a latency call of one fit.
The sizes below (4, 40, 64 / 128, 512) sit well away from every crossover.  The profile hook confirms the half it can see (a
latency call records trmm launches and no potf2 launch, the others the reverse), as tests/test_gpu_device_extents.py does.
Short fp64 windows (N <= 144, or 160 at d <= 2) run k_small_predict / k_small, whose ladder is inside the kernel; resident
windows run k_window_set_theta."""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_oracle as go
import failure_oracle as fo
from forecast_oracle import sliding_window_forecast
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu

TOL64 = 1e-6                 # BASELINE.json north_star, as tests/test_gpu_parity.py
TOL32, REFINED_MEAN32 = 1e-3, 5e-5   # the fp32 contract of include/corenav_gp.h: variance / logML max(1e-3, 10 x LAPACK's own error), refined mean 5e-5
DEV = "cuda:0"
MAXT = 10                    # CGP_MAX_THETA
N, D, M = fo.N_TILED, fo.D_TILED, fo.M_TILED
SE, BROWN, MAT52 = 1, 2, 4


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - b)) / max(np.max(np.abs(b)), 1e-300))


def releach(a, b):
    return float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))


def pad(theta):
    return np.pad(theta, (0, MAXT - len(theta)))


# ---- data ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def healthy(kid, n, d, m, b):
    """Healthy window number b of kernel kid: X (n, d), y (n,), Xs (m, d), theta."""
    seed = 9100 + 97 * n + 13 * d + b
    if kid == BROWN:
        t, y = synth.reference_window(n, 11 + 3 * (b % 40), seed)
        return t[:, None], y, (t[-1] + 1.0 + np.arange(m))[:, None], synth.theta_for(BROWN, 1, y)
    X, y, Xs = synth.window(n, d, m, seed)
    return X, y, Xs, synth.theta_for(SE, d, y, np.random.default_rng(seed + 7))       # SE-ARD's layout is the Matern pair's


@functools.lru_cache(maxsize=None)
def healthy_batch(kid, B, n, d, m):
    X, y, Xs, th = zip(*[healthy(kid, n, d, m, b) for b in range(B)])
    return np.stack(X), np.stack(y), np.stack(Xs), np.stack([pad(t) for t in th])


def with_failures(kid, B, n, d, m, bad):
    """The healthy batch with the fits of `bad` = {slot: (p, q)} (or {slot: (p, q, shift)} rung windows) replaced by lattice windows."""
    X, y, Xs, th = (a.copy() for a in healthy_batch(kid, B, n, d, m))
    for slot, pq in bad.items():
        if len(pq) == 3:
            X[slot], y[slot], t = fo.rung_window(kid, n, d, pq[0], pq[1], seed=slot, shift=pq[2])[:3]
        else:
            X[slot], y[slot], t = fo.lattice_window(kid, n, d, pq[0], pq[1], seed=slot)
        th[slot] = pad(t)
    return X, y, Xs, th


@functools.lru_cache(maxsize=None)
def oracle_of(kid, n, d, m, b):
    X, y, Xs, th = healthy(kid, n, d, m, b)
    f = fo.fit(kid, th, X, y)
    assert f.jitter == 0.0
    mu, var = fo.predict(f, Xs)
    e32 = fo.lapack_fp32_error(kid, th, X, y, Xs, f) if kid == SE else None
    return mu, var, f.logml, e32


def check_parity(kid, n, d, m, b, mean, var, logml, f32=False):
    omu, ovar, ologml, e32 = oracle_of(kid, n, d, m, b)
    errs = relmax(mean, omu), releach(var, ovar), abs(logml - ologml) / abs(ologml)
    bars = (REFINED_MEAN32, max(TOL32, 10.0 * e32), max(TOL32, 10.0 * e32)) if f32 else (TOL64,) * 3
    print("fit", b, "errors (mean, var, logml)", errs, "bars", bars)
    assert all(e < t for e, t in zip(errs, bars)), (b, errs, bars)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32 else np.float64)).to(DEV)


def schedule_class(ctx, call):
    """"latency" or "dense" (mid-size / throughput / full batch) from the per-kernel profile hook of one more call."""
    ctx.profile_enable(True)
    try:
        call()
        n = {k: v["launches"] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile_enable(False)
    return "latency" if n["trmm"] > 0 and n["potf2"] == 0 else "dense" if n["potf2"] > 0 and n["trmm"] == 0 else n


# ---- a. index and isolation per schedule, device entry ---------------------------------------------------------------------------
def fit_device(ctx, T, kid, X, y, Xs, th):
    """cgp_fit_predict_batch_device, djitter NULL (no ladder): (mean, var, logml, info) as numpy; dinfo prefilled with -7."""
    B, n, d = X.shape
    m = Xs.shape[1]
    dX, dy, dXs, dth = dev(X.transpose(0, 2, 1), T), dev(y, T), dev(Xs.transpose(0, 2, 1), T), dev(th, torch.float64)
    dmean, dvar = torch.zeros(B, m, dtype=T, device=DEV), torch.zeros(B, m, dtype=T, device=DEV)
    dlogml, dinfo = torch.zeros(B, dtype=torch.float64, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert ctx.fit_predict_batch_device(B, n, d, m, kid, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0, True,
                                        dmean.data_ptr(), dvar.data_ptr(), dlogml.data_ptr(), dinfo.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    return dmean.cpu().numpy(), dvar.cpu().numpy(), dlogml.cpu().numpy(), dinfo.cpu().numpy()


#             dtype  B    schedule at three block steps (module docstring)
SCHEDULES = [("F64", 4, "latency"),          # <= 28
             ("F64", 40, "dense"),           # mid-size: 28 < B <= 48
             ("F64", 64, "dense"),           # throughput, 48 < B < 512: the diagonal tile inside the panel launch
             ("F64", 512, "dense"),          # full batch, B >= FUSED64_BELOW = 512: separate diagonal launches
             ("F32", 4, "latency"),          # <= 24
             ("F32", 40, "dense"),           # mid-size, the fat diagonal form: 24 < B <= 96
             ("F32", 128, "dense")]          # throughput, the packed diagonal form: B > 96
CASES_A = [(dt, B, cls, SE) for dt, B, cls in SCHEDULES]
CASES_A += [("F64", B, cls, MAT52) for dt, B, cls in SCHEDULES if dt == "F64" and B in (4, 40, 64)]     # the Matern instantiations of the tile kernels
CASES_A += [("F64", B, cls, BROWN) for dt, B, cls in SCHEDULES if dt == "F64" and B in (4, 64)]


@pytest.mark.parametrize("dtype_name,B,cls,kid", CASES_A, ids=lambda v: str(v))
def test_failing_pivot_and_neighbours_on_every_schedule(engine, dtype_name, B, cls, kid):
    """Calls of B fits with failed fits at slots 0, B // 2, B - 1 (and 9 from eight fits), each at another position; the twelve
    (p, q) pairs of failure_oracle.POSITIONS are spread over the calls, so every position meets every schedule.  dinfo is p + 1 for
    the failed fits and 0 for all others; the healthy fits are bitwise those of the all-healthy control call; the first and the last
    of them meet the oracle (a call of four fits has one healthy fit: slot 1); the control call after the failing ones reports dinfo == 0 everywhere (no status survives a call) and is bitwise the
    control call before them.  fp32 runs under the default refinement (d = 3: every fit refined), so the refinement launches
    run over a failed factor beside healthy ones."""
    f32 = dtype_name == "F32"
    T = torch.float32 if f32 else torch.float64
    d = 1 if kid == BROWN else D
    slots = [0, B // 2, B - 1] + ([9] if B >= 8 else [])
    assert len(set(slots)) == len(slots) and len(fo.POSITIONS) % len(slots) == 0
    ctx = engine.Context(max_n=N, max_m=M, max_d=d, max_batch=B, dtype=getattr(engine, dtype_name))
    try:
        Xh, yh, Xsh, thh = healthy_batch(kid, B, N, d, M)
        control = fit_device(ctx, T, kid, Xh, yh, Xsh, thh)
        assert not control[3].any(), control[3]
        good = [b for b in range(B) if b not in slots]
        for b in (good[0], good[-1]):
            check_parity(kid, N, d, M, b, control[0][b], control[1][b], control[2][b], f32)
        for c in range(len(fo.POSITIONS) // len(slots)):
            bad = dict(zip(slots, fo.POSITIONS[c * len(slots):(c + 1) * len(slots)]))
            mean, var, logml, info = fit_device(ctx, T, kid, *with_failures(kid, B, N, d, M, bad))
            want = np.zeros(B, dtype=np.int32)
            for s, (p, _) in bad.items():
                want[s] = p + 1
            print("call", c, "bad", bad, "dinfo of the bad slots", info[slots])
            assert np.array_equal(info, want), (c, bad, np.flatnonzero(info != want), info[info != want], want[info != want])
            for k, (a, ref) in enumerate(zip((mean, var, logml), control)):
                assert np.array_equal(a[good], ref[good]), (c, "mean var logml".split()[k], [b for b in good if not np.array_equal(a[b], ref[b])])
        after = fit_device(ctx, T, kid, Xh, yh, Xsh, thh)
        assert not after[3].any(), after[3]
        assert all(np.array_equal(a, b) for a, b in zip(after, control))
        got = schedule_class(ctx, lambda: fit_device(ctx, T, kid, Xh, yh, Xsh, thh))
        assert got == cls, (dtype_name, B, got)
    finally:
        ctx.close()


# ---- b. host entry points: the ladder runs out at the same pivot ------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(128, 64), (263, 131)])
def test_fit_reports_the_pivot_after_the_ladder_and_no_jitter(engine, p, q):
    """cgp_fit (always the tiled path): six factorisations, jitter 0 and five rungs, each failing at row p; the return value is
    p + 1 and cgp_last_jitter is 0 after a failed fit (include/corenav_gp.h), also when the fit before it had needed a rung."""
    ctx = engine.Context(max_n=N, max_m=M, max_d=D)
    try:
        X, y, th, k, jitter = fo.rung_window(SE, N, D, 192, 96)
        rc, _ = ctx.fit(X, y, SE, th)
        assert rc == 0 and ctx.last_jitter() == pytest.approx(jitter, rel=1e-12)
        X, y, th = fo.lattice_window(SE, N, D, p, q)
        rc, _ = ctx.fit(X, y, SE, th)
        assert rc == p + 1
        assert ctx.last_jitter() == 0.0
        with pytest.raises(engine.CgpError):
            ctx.predict(np.zeros((2, D)))              # no fitted model after a failed fit
    finally:
        ctx.close()


@pytest.mark.parametrize("p,q", [(128, 64), (263, 131)])
def test_fit_predict_batch_exhausts_the_ladder_at_the_same_pivot(engine, p, q):
    """cgp_fit_predict_batch of five fits, one hopeless: it is retried alone on five rungs and fails at row p on each; the return
    value and its info are p + 1, the other four are bitwise those of the control call."""
    B, bad = 5, 2
    ctx = engine.Context(max_n=N, max_m=M, max_d=D, max_batch=B)
    try:
        Xh, yh, Xsh, thh = healthy_batch(SE, B, N, D, M)
        rc0, m0, v0, l0, i0 = ctx.fit_predict_batch(Xh, yh, Xsh, thh[:, :D + 2], SE)
        assert rc0 == 0 and not i0.any()
        X, y, Xs, th = with_failures(SE, B, N, D, M, {bad: (p, q)})
        rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th[:, :D + 2], SE)
        assert rc == p + 1 and list(info) == [0, 0, p + 1, 0, 0]
        good = [0, 1, 3, 4]
        assert np.array_equal(mean[good], m0[good]) and np.array_equal(var[good], v0[good]) and np.array_equal(logml[good], l0[good])
        for b in (0, 4):
            check_parity(SE, N, D, M, b, mean[b], var[b], logml[b])
    finally:
        ctx.close()


@pytest.mark.parametrize("kid,n,d", [(SE, 144, 3), (SE, 37, 1), (BROWN, 144, 1), (BROWN, 37, 1)])
def test_short_windows_report_the_pivot_from_the_in_kernel_ladder(engine, kid, n, d):
    """cgp_fit_predict_batch of short fp64 windows: k_small_predict, one launch, the ladder inside the kernel.  Four failed fits
    at rows 1, 16, 17 and n - 1 beside two healthy ones."""
    B, m = 6, 20
    bad = dict(zip([0, 2, 3, 5], [(p, p // 2) for p in fo.short_positions(n)]))
    nth = 4 if kid == BROWN else d + 2
    ctx = engine.Context(max_n=n, max_m=m, max_d=d, max_batch=B)
    try:
        Xh, yh, Xsh, thh = healthy_batch(kid, B, n, d, m)
        rc0, m0, v0, l0, i0 = ctx.fit_predict_batch(Xh, yh, Xsh, thh[:, :nth], kid)
        assert rc0 == 0 and not i0.any()
        X, y, Xs, th = with_failures(kid, B, n, d, m, bad)
        rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th[:, :nth], kid)
        want = [bad[b][0] + 1 if b in bad else 0 for b in range(B)]
        assert list(info) == want and rc == want[0], (rc, info, want)
        for b in (1, 4):
            assert np.array_equal(mean[b], m0[b]) and np.array_equal(var[b], v0[b]) and logml[b] == l0[b]
            check_parity(kid, n, d, m, b, mean[b], var[b], logml[b])
        rc, _, _, _, info = ctx.fit_predict_batch(Xh, yh, Xsh, thh[:, :nth], kid)
        assert rc == 0 and not info.any()
    finally:
        ctx.close()


@pytest.mark.parametrize("n,p", [(144, 1), (144, 16), (144, 17), (144, 143), (N, 128), (N, 263)])
def test_nll_grad_reports_the_pivot(engine, n, p):
    """cgp_nll_grad: k_small (n = 144) and the gradient-mode tiled factorisation (n = 264; max_m >= n)."""
    ctx = engine.Context(max_n=n, max_m=n, max_d=D)
    try:
        X, y, th = fo.lattice_window(SE, n, D, p, p // 2)
        with pytest.raises(engine.CgpError) as ei:
            ctx.nll_grad(X, y, SE, th)
        assert ei.value.code == p + 1
        assert ctx.last_jitter() == 0.0
        Xh, yh, _, thh = healthy(SE, n, D, M, 0)
        nll, g = ctx.nll_grad(Xh, yh, SE, thh)             # the context is usable, and nothing of the failure is left in it
        onll, og = go.nll_and_grad(SE, thh, Xh, yh)
        assert abs(nll - onll) <= TOL64 * abs(onll) and np.max(np.abs(g - og)) <= TOL64 * np.max(np.abs(og))
    finally:
        ctx.close()


# ---- c. derived paths with the failure beyond tile 0 -------------------------------------------------------------------------------
P_MULTI, B_DER, BAD_DER, POS_DER = 3, 5, 2, (192, 96)


@pytest.fixture(scope="module")
def ctx_derived(engine):
    c = engine.Context(max_n=N, max_m=N, max_d=D, max_batch=B_DER)       # max_m >= N: the gradient-mode calls
    c.joint_reserve(B_DER, M)
    c.multi_reserve(B_DER, P_MULTI)
    c.multi_grad_reserve(B_DER, P_MULTI)
    yield c
    c.close()


def targets(y):
    """Y (B, P, N): column 0 is y, the others y plus seeded noise."""
    Y = y[:, None, :] + 0.02 * np.random.default_rng(3).normal(size=(y.shape[0], P_MULTI, y.shape[1]))
    Y[:, 0] = y
    return Y


def derived_pair(run):
    """run(X, y, Xs, th) -> dict of numpy outputs with "info".  The control call, the call with the failed fit (dinfo 193 in its
    slot; the healthy fits' rows bitwise the control's -- what the failed fit's own rows hold beyond the NaN the header promises
    is unspecified and not looked at), and the control call again: nothing of the failure is left in the context."""
    control = run(*healthy_batch(SE, B_DER, N, D, M))
    assert not control["info"].any()
    out = run(*with_failures(SE, B_DER, N, D, M, {BAD_DER: POS_DER}))
    assert list(out["info"]) == [0, 0, POS_DER[0] + 1, 0, 0], out["info"]
    good = [b for b in range(B_DER) if b != BAD_DER]
    for k in control:
        assert np.array_equal(out[k][good], control[k][good]), k
        assert np.all(np.isfinite(control[k]))
    again = run(*healthy_batch(SE, B_DER, N, D, M))
    assert all(np.array_equal(again[k], control[k]) for k in control)
    return out


def zeros(*shape):
    return torch.zeros(*shape, dtype=torch.float64, device=DEV)


def test_loo_batch_device_failure_beyond_tile_0(ctx_derived):
    F = torch.float64

    def run(X, y, Xs, th):
        o = {k: zeros(B_DER, N) for k in ("loo_mean", "loo_var", "loo_lpd")}
        o.update(lpd_sum=zeros(B_DER), logml=zeros(B_DER), info=torch.full((B_DER,), -7, dtype=torch.int32, device=DEV))
        dX, dy, dth = dev(X.transpose(0, 2, 1), F), dev(y, F), dev(th, F)
        torch.cuda.synchronize()
        assert ctx_derived.loo_batch_device(B_DER, N, D, SE, dX.data_ptr(), dy.data_ptr(), dth.data_ptr(), 0, o["loo_mean"].data_ptr(),
                                            o["loo_var"].data_ptr(), o["loo_lpd"].data_ptr(), o["lpd_sum"].data_ptr(),
                                            o["logml"].data_ptr(), o["info"].data_ptr(), 0) == 0
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}
    out = derived_pair(run)
    for k in ("loo_mean", "loo_var", "loo_lpd", "lpd_sum"):
        assert np.all(np.isnan(out[k][BAD_DER])), k


def test_fit_predict_cov_batch_device_failure_beyond_tile_0(ctx_derived):
    F = torch.float64

    def run(X, y, Xs, th):
        o = dict(mean=zeros(B_DER, M), cov=zeros(B_DER, M, M), logml=zeros(B_DER), info=torch.full((B_DER,), -7, dtype=torch.int32, device=DEV))
        dX, dy, dXs, dth = dev(X.transpose(0, 2, 1), F), dev(y, F), dev(Xs.transpose(0, 2, 1), F), dev(th, F)
        torch.cuda.synchronize()
        assert ctx_derived.fit_predict_cov_batch_device(B_DER, N, D, M, SE, dX.data_ptr(), dy.data_ptr(), dXs.data_ptr(), dth.data_ptr(), 0,
                                                        True, o["mean"].data_ptr(), o["cov"].data_ptr(), o["logml"].data_ptr(),
                                                        o["info"].data_ptr(), 0) == 0
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}
    out = derived_pair(run)
    assert np.all(np.isnan(out["cov"][BAD_DER]))


def test_fit_predict_multi_batch_device_failure_beyond_tile_0(ctx_derived):
    F = torch.float64

    def run(X, y, Xs, th):
        o = dict(mean=zeros(B_DER, P_MULTI, M), var=zeros(B_DER, M), logml=zeros(B_DER, P_MULTI),
                 info=torch.full((B_DER,), -7, dtype=torch.int32, device=DEV))
        dX, dY, dXs, dth = dev(X.transpose(0, 2, 1), F), dev(targets(y), F), dev(Xs.transpose(0, 2, 1), F), dev(th, F)
        torch.cuda.synchronize()
        assert ctx_derived.fit_predict_multi_batch_device(B_DER, N, D, M, P_MULTI, SE, dX.data_ptr(), dY.data_ptr(), dXs.data_ptr(),
                                                          dth.data_ptr(), 0, True, o["mean"].data_ptr(), o["var"].data_ptr(),
                                                          o["logml"].data_ptr(), o["info"].data_ptr(), 0) == 0
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}
    out = derived_pair(run)
    for k in ("mean", "var", "logml"):
        assert np.all(np.isnan(out[k][BAD_DER])), k


def test_multi_nll_grad_batch_device_failure_beyond_tile_0(ctx_derived):
    F = torch.float64
    nth = D + 2

    def run(X, y, Xs, th):
        o = dict(nll=zeros(B_DER), grad=zeros(B_DER, nth), logml=zeros(B_DER, P_MULTI),
                 info=torch.full((B_DER,), -7, dtype=torch.int32, device=DEV))
        dX, dY, dth = dev(X.transpose(0, 2, 1), F), dev(targets(y), F), dev(th, F)
        torch.cuda.synchronize()
        assert ctx_derived.multi_nll_grad_batch_device(B_DER, N, D, P_MULTI, SE, dX.data_ptr(), dY.data_ptr(), dth.data_ptr(), 0,
                                                       o["nll"].data_ptr(), o["grad"].data_ptr(), nth, o["logml"].data_ptr(),
                                                       o["info"].data_ptr(), 0) == 0
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}
    out = derived_pair(run)
    for k in ("nll", "grad", "logml"):
        assert np.all(np.isnan(out[k][BAD_DER])), k


# ---- d. resident windows -----------------------------------------------------------------------------------------------------------
def window_data(n, p, start, T):
    """Three windows of d = 3, T ticks: 0 and 2 seeded random streams, 1 the lattice in which tick start + p repeats the input of
    tick start + p // 2 -- position p of the window that holds ticks [start, start + n)."""
    W = 3
    X, y, theta = np.zeros((W, T, D)), np.zeros((W, T)), np.zeros((W, D + 2))
    for w in (0, 2):
        rng = np.random.default_rng(400 + w)
        t = np.arange(11, 11 + T, dtype=np.float64)
        X[w] = np.column_stack([(t - t.mean()) / t.std(), rng.normal(size=T), rng.normal(size=T)])
        y[w] = synth._slip_series(rng, t)
        theta[w] = np.concatenate([[0.02], np.linspace(0.8, 1.6, D), [1e-3]])
    Xl, yl, th = fo.lattice_window(SE, T, D, start + p, start + p // 2, seed=1)
    X[1], y[1], theta[1] = Xl, yl, th
    theta[1, -1] = fo.SHIFT                        # pushed under POSITIVE noise: the pair's block is [[1.05, 1], [1, 1.05]]
    bad = theta.copy()
    bad[1, -1] = th[-1]                            # -0.05 - 1e-8
    return X, y, theta, bad


@pytest.mark.parametrize("n,p,start", fo.WINDOWS, ids=lambda v: str(v))
def test_window_set_theta_reports_the_pivot_in_window_order(engine, n, p, start):
    """cgp_window_set_theta with a theta under which window 1 fails at position p of its own order (oldest sample first), before
    and after the ring has wrapped (start = 23 ticks pushed beyond n); windows 0 and 2 untouched bit for bit; the window is then
    revived with the healthy theta and forecasts in parity with a refit."""
    T, Mw = n + start, 12
    X, y, theta, bad = window_data(n, p, start, T)
    # the window's own samples as the CPU test saw them: lattice points [start, start + n) with the pair at (p, p // 2)
    Xc, _, thc = fo.lattice_window(SE, n, D, p, p // 2, start=start)
    assert np.array_equal(X[1, start:], Xc) and np.array_equal(bad[1], thc)
    rng = np.random.default_rng(5)
    Xs = np.stack([X[w, rng.integers(start, T, size=Mw)] + 0.3 * theta[w, 1:1 + D] * rng.normal(size=(Mw, D)) for w in range(3)])
    ctx = engine.Context(max_n=8, max_m=8, max_d=D)
    try:
        ctx.window_init(3, n, D, SE, theta)
        ctx.window_push(X, y)
        assert [ctx.window_state(w) for w in range(3)] == [(n, 0)] * 3
        m0, v0 = ctx.window_predict(Xs)
        logml, info, rc = ctx.window_set_theta(bad, select=[0, 1, 0], check=False)
        assert rc == 2 and list(info) == [0, p + 1, 0] and np.isnan(logml[1]), (rc, info, logml)
        assert ctx.window_state(1) == (n, p + 1) and ctx.window_state(0) == (n, 0) and ctx.window_state(2) == (n, 0)
        m1, v1, code = ctx.window_predict(Xs, check=False)
        assert code == p + 1 and np.all(np.isnan(m1[1])) and np.all(np.isnan(v1[1]))
        for w in (0, 2):
            assert np.array_equal(m1[w], m0[w]) and np.array_equal(v1[w], v0[w])
        logml, info = ctx.window_set_theta(theta, select=[0, 1, 0])
        assert not info.any() and ctx.window_state(1) == (n, 0)
        m2, v2 = ctx.window_predict(Xs)
        omu, ovar = sliding_window_forecast(SE, theta[1], n, X[1], y[1], Xs[1])
        assert relmax(m2[1], omu) < TOL64 and releach(v2[1], ovar) < TOL64
        for w in (0, 2):
            assert np.array_equal(m2[w], m0[w]) and np.array_equal(v2[w], v0[w])
    finally:
        ctx.close()


# ---- 3. a rung that is needed, beyond tile 0 ---------------------------------------------------------------------------------------
def test_fit_takes_the_rung_the_window_needs(engine):
    """The duplicate at row 192 with sigma_n^2 + 1e-8 = -3e-5: positive definite from rung k = 2 (1e-4 mean(diag)) only."""
    X, y, th, k, jitter = fo.rung_window(SE, N, D, 192, 96)
    Xs = X[::13][:M] + 0.3 * th[1:1 + D] * np.random.default_rng(8).normal(size=(M, D))
    ctx = engine.Context(max_n=N, max_m=M, max_d=D)
    try:
        rc, logml = ctx.fit(X, y, SE, th)
        f = go.fit(SE, th, X, y)
        assert k == 2 and rc == 0 and ctx.last_jitter() == pytest.approx(f.jitter, rel=1e-12) and f.jitter == pytest.approx(jitter, rel=1e-12)
        mean, var = ctx.predict(Xs)
        omu, ovar = go.predict(f, Xs)
        assert relmax(mean, omu) < TOL64 and releach(var, ovar) < TOL64 and abs(logml - f.logml) <= TOL64 * abs(f.logml)
    finally:
        ctx.close()


def test_batch_ladder_gives_each_fit_its_own_rung_on_the_mid_size_schedule(engine):
    """cgp_fit_predict_batch of 40 fits (mid-size): two fits need different rungs (k = 1 and k = 3), each is retried alone; info is 0
    everywhere, the two meet the oracle at 1e-5 (the bar of test_batch_jitter_retry_is_per_fit), the other 38 are bitwise those
    of the control call."""
    B, bad = 40, {7: (192, 96, 3e-6), 31: (192, 96, 3e-4)}
    ctx = engine.Context(max_n=N, max_m=M, max_d=D, max_batch=B)
    try:
        Xh, yh, Xsh, thh = healthy_batch(SE, B, N, D, M)
        rc0, m0, v0, l0, i0 = ctx.fit_predict_batch(Xh, yh, Xsh, thh[:, :D + 2], SE)
        assert rc0 == 0 and not i0.any()
        X, y, Xs, th = with_failures(SE, B, N, D, M, bad)
        for s in bad:                                  # test points where the lattice window has something to say
            Xs[s] = X[s, ::13][:M] + 0.3 * th[s, 1:1 + D] * np.random.default_rng(s).normal(size=(M, D))
        rc, mean, var, logml, info = ctx.fit_predict_batch(X, y, Xs, th[:, :D + 2], SE)
        assert rc == 0 and not info.any(), (rc, info)
        good = [b for b in range(B) if b not in bad]
        assert np.array_equal(mean[good], m0[good]) and np.array_equal(var[good], v0[good]) and np.array_equal(logml[good], l0[good])
        for s, (_, _, shift) in bad.items():
            f = go.fit(SE, th[s, :D + 2], X[s], y[s])
            assert f.jitter == pytest.approx(fo.rung_of(shift)[1], rel=1e-12)
            omu, _ = go.predict(f, Xs[s])
            assert relmax(mean[s], omu) < 1e-5 and abs(logml[s] - f.logml) < 1e-5 * abs(f.logml)
    finally:
        ctx.close()
