"""The extents of every caller buffer of the `*_device` entry points (include/corenav_gp.h, "device buffers"), on guard-band
allocations (tests/guarded.py).  The kernels behind these calls work in padded shapes -- 128-row tiles, 16-column panels, M
rounded up to 16, 64- or 128-target tiles, window slabs rounded up to 16, the short-window kernel's thread-strided stores --
while the header states the extents in real shapes.  Every case carves ALL arguments of its call out of one allocation, each
between two 64 KiB guards, and asserts

  a. nothing outside is written: after the call every guard, every input (dX, dy, dY, dXs, dtheta, djitter, dxi, dselect, dxs,
     dys) and every gap column [ntheta, stride) of a strided array is bit-identical;
  b. everything inside is written, from the arguments only: the call runs on (1) guards and output prefill 0xFF (NaN as fp64 /
     fp32, -1 as int32), (2) guards and prefill 0x3F (a finite value), (3) every region one element off its 256-byte alignment
     and (4) separate plain tensors, the route the rest of the suite pins to the oracle.  The documented outputs of the four
     runs are bitwise equal (torch.equal on the raw bytes: no tolerance anywhere) and none holds a prefill pattern;
  c. optional outputs: with each NULL-able output passed as 0 the others are bitwise unchanged, the unpassed region untouched;
  d. a failure stays inside: the last fit / window of the call is made non-positive-definite; its NaN covers its own rows
     where the header promises NaN, the neighbours' rows and every guard are bitwise those of the run without the failure.

Which schedule a fit case reaches is ASSERTED (test_fit_cases_reach_the_schedules_named, with cgp_profile_enable /
cgp_profile_read: the one-launch short-window kernel records no launch, the latency schedule records k_trmm_sk launches and no
potf2 launch, the mid-size and throughput schedules a potf2 launch and no trmm launch).  What is expected there, from
fit_predict_device, small_batch_predict_ok of csrc/cgp_engine.hip and sched_plan of csrc/cgp_sched_plan.hpp as they stand:
  - cgp_fit_predict_batch_device and the sweep in fp64, SE and RBF x Brownian kernels: N <= 144 for any d, N <= 160 at d <= 2
    (SM_MAX_NB = 10 blocks of 16 and the LDS bound) and M > 0 run k_small_predict -- (3, 15, 20) AND (3, 129, 17).  The issue's
    "tiled, two block steps, latency schedule" is therefore reached in fp64 by (3, 161, 17) -- the shortest window that is tiled at
    every d, 33 rows into the second tile --, by Matern on (3, 129, 17) (no short-window form), by every fp32 case (an fp32
    context has no short-window kernel) and by the joint, multi-target and leave-one-out calls (tiled for every N).
  - tiled calls, NT = ceil(N / 128) block steps: the latency schedule takes batch <= min(lat_fits_by_steps(fp64, NT), lat_cap) --
    48 (fp64) / 32 (fp32) fits at NT <= 2, 28 / 24 at NT <= 4; lat_cap = min(48, max_batch) -- if also batch x (NT + ET + 1) <=
    lat_units and, from three block steps, batch <= lat_img_fits: both slabs are sized at cgp_create for the most fits the
    schedule takes at any NT the context can see, so a call of 3 fits is far inside them.  The mid-size form takes batch <=
    min(mid_fits(NT), mid_cap): 48 in fp64 below six block steps, 96 in fp32, mid_cap = min(96, max_batch).  N = 161 has two block
    steps, so 49 fp64 fits (context of 49) and 97 fp32 fits (context of 97) are one past both: the throughput schedule, k_panel.
    The profile hook cannot tell mid-size from throughput; that half rests on the two numbers above.
  - the sweep cuts 49 fits into shards of 25 and 24 on contexts of their own: each is a latency-schedule call.
The RBF x Brownian tick-grid table (tab_n of k_small_predict) is NOT reachable from any *_device form: fit_predict_device passes
the table length the host-buffer entry point left behind, and a device call has none ("only the host-buffer entry point knows
whether the inputs are tick counts").  The kid = 2 cases here run the direct evaluation: k_small_predict<true, 1> at (3, 129, 17),
the tiled Gram path of the latency schedule at (3, 161, 17).
Which kernel a window push reaches is asserted with cgp_debug_window_plan (test_window_push_cases_reach_...)."""
import functools

import numpy as np
import pytest
import torch

from guarded import Slab, itemsize
import corenav_gp_amd.synth as synth

pytestmark = pytest.mark.gpu

F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8
NP = {F64: np.float64, F32: np.float32, I32: np.int32, U8: np.uint8}
DEV = "cuda:0"
MAXT = 10   # CGP_MAX_THETA


# ---- module-wide contexts -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


@pytest.fixture(scope="module")
def ctx64(engine):
    c = engine.Context(max_n=257, max_m=257, max_d=3, max_batch=49)     # max_m >= N: the gradient-mode calls
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx32(engine):
    c = engine.Context(max_n=257, max_m=130, max_d=3, max_batch=97, dtype=engine.F32)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sweep(engine):
    s = engine.Sweep([0, 0], 257, 130, 3, 49)
    yield s
    s.close()


@pytest.fixture(scope="module")
def wctx(engine):
    c = engine.Context(max_n=8, max_m=8, max_d=2)       # the windows bring their own buffers
    yield c
    c.close()


# ---- a call as a list of regions ------------------------------------------------------------------------------------------------
class R:
    """One pointer argument.  data: an input (numpy array).  keep: elements of an output that the call must not write (gap
    columns, unselected windows).  optional: may be passed as 0.  nan: NaN on the failing row where the header promises it.
    rowfail: the LAST row of this output belongs to the fit / window that is made to fail."""

    def __init__(self, name, dtype, shape, data=None, keep=None, optional=False, nan=False, rowfail=True):
        self.name, self.dtype, self.shape = name, dtype, tuple(int(s) for s in shape)
        self.data = None if data is None else np.ascontiguousarray(data, dtype=NP[dtype]).reshape(self.shape)
        self.keep = None if keep is None else np.ascontiguousarray(np.broadcast_to(np.asarray(keep, dtype=bool), self.shape))
        self.optional, self.nan, self.rowfail = optional, nan, rowfail

    def doc(self, t, rows=slice(None)):
        """The documented elements of output tensor t (optionally of some rows only) as raw bytes, one row per element."""
        m = np.ones(self.shape, dtype=bool) if self.keep is None else ~self.keep
        sel = np.zeros(self.shape, dtype=bool)
        sel[rows] = m[rows]
        v = t[torch.from_numpy(sel)].contiguous()
        return v.view(U8).view(v.numel(), itemsize(self.dtype)), v


def IN(name, dtype, arr):
    return R(name, dtype, np.shape(arr), data=arr)


class Case:
    def __init__(self, regions, call, zero=(), nonzero_on_fail=(), sync=None):
        self.regions, self.call, self.zero, self.nonzero_on_fail, self.sync = regions, call, zero, nonzero_on_fail, sync
        self.outputs = [r for r in regions if r.data is None]


def finish(case):
    if case.sync:
        case.sync()
    torch.cuda.synchronize()


def run_slab(case, byte, misalign=0, omit=(), prefill_check=True):
    """The call on one slab: guards and output prefill `byte`.  Asserts (a) and the prefill half of (b); returns the outputs."""
    slab = Slab(DEV)
    for r in case.regions:
        if r.data is not None:
            slab.region(r.name, r.dtype, r.shape, misalign, role="input")
        else:
            slab.region(r.name, r.dtype, r.shape, misalign, keep=True if r.name in omit else r.keep)
    slab.fill_guards(byte)
    for r in case.regions:
        if r.data is not None:
            slab.view(r.name).copy_(torch.from_numpy(r.data))
        else:
            slab.fill(r.name, byte)
    torch.cuda.synchronize()
    snap = slab.snapshot()
    case.call({r.name: 0 if r.name in omit else slab.ptr(r.name) for r in case.regions})
    finish(case)
    touched = slab.check(snap)
    print("protected bytes that changed (region, side, first offset, bytes):", touched)
    assert touched == [], touched
    outs = {r.name: slab.view(r.name).cpu().clone() for r in case.outputs if r.name not in omit}
    if prefill_check:
        for r in case.outputs:
            if r.name in outs:
                raw, _ = r.doc(outs[r.name])
                left = int((raw == byte).all(dim=1).sum())
                assert left == 0, (r.name, "documented elements never written", left)
    return outs


def run_plain(case):
    """The existing style: every argument a tensor of its own (the reference of the bitwise comparisons)."""
    t = {r.name: torch.from_numpy(r.data).to(DEV) if r.data is not None else torch.zeros(r.shape, dtype=r.dtype, device=DEV)
         for r in case.regions}
    torch.cuda.synchronize()
    case.call({k: v.data_ptr() for k, v in t.items()})
    finish(case)
    return {r.name: t[r.name].cpu() for r in case.outputs}


def assert_same(case, outs, ref, what, rows=None):
    for r in case.outputs:
        if r.name not in outs:
            continue
        sel = slice(None) if rows is None or not r.rowfail else rows
        a, _ = r.doc(outs[r.name], sel)
        b, _ = r.doc(ref[r.name], sel)
        assert torch.equal(a, b), (what, r.name, int((a != b).any(dim=1).sum()), "elements differ")


def check_case(build):
    """build(mode) -> Case for mode "normal", "base" (the call the failing one is compared with) and "fail"."""
    case = build("normal")
    ref = run_plain(case)
    for r in case.outputs:
        if r.name in case.zero:
            assert not ref[r.name].any(), (r.name, ref[r.name])
    assert_same(case, run_slab(case, 0xFF), ref, "guards 0xFF")
    assert_same(case, run_slab(case, 0x3F), ref, "guards 0x3F")
    assert_same(case, run_slab(case, 0xFF, misalign=1), ref, "misaligned")
    for r in case.outputs:
        if r.optional:
            assert_same(case, run_slab(case, 0xFF, omit=(r.name,)), ref, "without " + r.name)
    base, fail = build("base"), build("fail")
    if fail is None:
        return
    ob = run_slab(base, 0xFF)
    of = run_slab(fail, 0xFF, prefill_check=False)
    assert_same(fail, of, ob, "neighbours of the failure", rows=slice(0, -1))
    for r in fail.outputs:
        last = slice(-1, None) if r.rowfail else slice(0, 0)
        if not r.nan and r.rowfail:   # no NaN promised (include/corenav_gp.h: the content of such a row is unspecified): a figure, not a bar
            raw, _ = r.doc(of[r.name], last)
            print("failing row of", r.name, ":", int((raw == 0xFF).all(dim=1).sum()), "of", raw.shape[0], "elements still hold the prefill")
        if r.nan:
            _, v = r.doc(of[r.name], last)
            assert v.numel() > 0 and torch.isnan(v).all(), (r.name, v)
        if r.name in fail.nonzero_on_fail:
            _, v = r.doc(of[r.name], last)
            assert v.numel() > 0 and (v != 0).all() and (v != -1).all(), (r.name, v)


# ---- the checker itself, once on the device --------------------------------------------------------------------------------------
def test_control_a_store_past_a_region_is_reported_on_the_device():
    slab = Slab(DEV)
    slab.region("dX", F64, (3, 2, 15), role="input")
    slab.region("dmean", F64, (3, 20))
    slab.region("dgrad", F64, (3, 8), keep=np.arange(8) >= 5)
    slab.fill_guards(0xFF)
    slab.view("dX").copy_(torch.arange(90, dtype=F64).view(3, 2, 15))
    slab.fill("dmean", 0xFF)
    slab.fill("dgrad", 0xFF)
    torch.cuda.synchronize()
    snap = slab.snapshot()
    slab.view("dmean").copy_(torch.rand(3, 20, dtype=F64))
    slab.view("dgrad")[:, :5] = 0.5
    torch.cuda.synchronize()
    assert slab.check(snap) == []
    r = slab.regions["dmean"]
    idx = torch.arange(r.end, r.end + 8, device=DEV)     # one double past the last fit's row: inside the slab's own allocation
    slab.buf[idx] = 0
    slab.view("dgrad")[2, 5] = 0.5
    slab.view("dX")[0, 0, 0] = float(np.frombuffer(bytes([0x11] * 8), dtype=np.float64)[0])
    torch.cuda.synchronize()
    assert slab.check(snap) == [("dX", "input", 0, 8), ("dmean", "after", 0, 8), ("dgrad", "gap", (2 * 8 + 5) * 8, 8)]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def nth_of(kid, d):
    return 4 if kid == 2 else d + 2


@functools.lru_cache(maxsize=None)
def fit_data(B, N, d, M, kid, fail):
    """B seeded windows: X (B, N, d), y (B, N), Xs (B, M, d), theta (B, CGP_MAX_THETA).  fail: the last fit gets duplicated
    inputs and a noise variance a hair below zero (the recipe of test_batch_jitter_retry_is_per_fit): not positive definite."""
    Xl, yl, Xsl, thl = [], [], [], []
    for b in range(B):
        seed = 7000 + 131 * N + 17 * d + b
        if kid == 2:     # RBF x Brownian on raw tick counts (synth.reference_window), the test ticks follow the window
            t, y = synth.reference_window(N, 11 + 3 * b, seed)
            X, Xs = t[:, None], (t[-1] + 1.0 + np.arange(M))[:, None]
            th = synth.theta_for(2, 1, y)
        else:
            X, y, Xs = synth.window(N, d, M, seed)
            th = synth.theta_for(1, d, y, np.random.default_rng(seed + 7))
        Xl.append(X); yl.append(y); Xsl.append(Xs); thl.append(np.pad(th, (0, MAXT - len(th))))
    X, y, Xs, th = np.stack(Xl), np.stack(yl), np.stack(Xsl), np.stack(thl)
    if fail:
        X[-1] = np.repeat(X[-1][:(N + 1) // 2], 2, axis=0)[:N]
        k00 = th[-1, 0] * (th[-1, 2] * X[-1, 0, 0] if kid == 2 else 1.0)
        th[-1, nth_of(kid, d) - 1] = -1e-8 - 1e-4 * k00
    return X, y, Xs, th


def fit_regions(T, B, N, d, M, kid, mode, tag=""):
    """The arguments every fit call shares, SoA per fit.  djitter: small per-fit values in the normal runs (the input is read),
    NULL beside the failing fit (the recipe: no jitter rescues it)."""
    X, y, Xs, th = fit_data(B, N, d, M, kid, mode == "fail")
    regs = [IN("dX" + tag, T, X.transpose(0, 2, 1)), IN("dy" + tag, T, y), IN("dXs" + tag, T, Xs.transpose(0, 2, 1)),
            IN("dtheta" + tag, F64, th)]
    if mode == "normal":
        regs.append(IN("djitter" + tag, F64, 1e-9 * (np.arange(B) % 3)))
    return regs


def jit(p, tag=""):
    return p.get("djitter" + tag, 0)


# ---- fits ------------------------------------------------------------------------------------------------------------------------
FIT64 = [(3, 15, 20), (3, 129, 17), (3, 161, 17), (3, 257, 130), (49, 161, 33)]
FIT32 = [(3, 15, 20), (3, 129, 17), (3, 257, 130), (97, 161, 33)]
FIT64_CASES = [(s, d, 1) for s in FIT64 for d in (1, 3)] + [((3, 129, 17), 1, 2), ((3, 161, 17), 1, 2), ((3, 129, 17), 1, 4),
                                                            ((3, 129, 17), 3, 4)]
SMALL, LATENCY, DENSE = "one launch", "latency", "mid-size / throughput"


def expected_schedule(f64, B, N, d, kid, tiled_only=False, lat_cap=48):
    """The module docstring's derivation as a function (what the profile hook is then asked to confirm)."""
    if f64 and not tiled_only and kid < 3 and N <= (160 if d <= 2 else 144):
        return SMALL
    NT = -(-N // 128)
    lat = (48 if f64 else 32) if NT <= 2 else (28 if f64 else 24)       # lat_fits_by_steps up to four block steps
    assert NT <= 4
    return LATENCY if B <= min(lat, lat_cap) else DENSE


def observed_schedule(prof):
    n = {k: v["launches"] for k, v in prof.items()}
    if not any(n.values()):
        return SMALL
    if n["trmm"] > 0 and n["potf2"] == 0:
        return LATENCY
    if n["potf2"] > 0 and n["trmm"] == 0:
        return DENSE
    return n


def ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def fit_predict_case(ctx, T, B, N, d, M, kid):
    def build(mode):
        regs = fit_regions(T, B, N, d, M, kid, mode) + [R("dmean", T, (B, M)), R("dvar", T, (B, M)), R("dlogml", F64, (B,)),
                                                        R("dinfo", I32, (B,))]

        def call(p):
            assert ctx.fit_predict_batch_device(B, N, d, M, kid, p["dX"], p["dy"], p["dXs"], p["dtheta"], jit(p), True, p["dmean"],
                                                p["dvar"], p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    return build


@pytest.mark.parametrize("shape,d,kid", FIT64_CASES, ids=ids)
def test_fit_predict_batch_device_fp64(ctx64, shape, d, kid):
    """SE-ARD on every shape.  RBF x Brownian on (3, 129, 17) (the short-window kernel's Brownian form) and on (3, 161, 17) (the
    Brownian Gram path of the tiled latency schedule meets a tail); Matern 5/2 on (3, 129, 17) (the MAT Gram path, tiled: one row
    into the second tile).  The tick-grid table is out of the device forms' reach (module docstring)."""
    B, N, M = shape
    check_case(fit_predict_case(ctx64, F64, B, N, d, M, kid))


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("shape", FIT32, ids=ids)
def test_fit_predict_batch_device_fp32(ctx32, shape, d):
    """dX / dy / dXs / dmean / dvar are 4-byte elements here, dtheta / djitter / dlogml stay fp64: a store of the wrong width
    shows in the byte-wise guards on either side of dmean and dvar."""
    B, N, M = shape
    check_case(fit_predict_case(ctx32, F32, B, N, d, M, 1))


def profiled(ctx_handles, lib, case, sync=None):
    """The launches per kernel class that one call of `case` records on each of the contexts."""
    import ctypes
    for h in ctx_handles:
        assert lib.cgp_profile_enable(h, 1) == 0
    try:
        run_plain(case)
        out = []
        for h in ctx_handles:
            ms, fl, n = np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64)
            dp = ctypes.POINTER(ctypes.c_double)
            assert lib.cgp_profile_read(h, ms.ctypes.data_as(dp), fl.ctypes.data_as(dp), n.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))) == 0
            out.append({k: {"launches": int(n[i])} for i, k in enumerate(("update", "potf2", "trmm", "finalize", "alpha"))})
        return out
    finally:
        for h in ctx_handles:
            assert lib.cgp_profile_enable(h, 0) == 0


def test_fit_cases_reach_the_schedules_named(engine, ctx64, ctx32, sweep):
    """Every fit case of this file through the per-kernel profile hook: the class of schedule it records is the one the module
    docstring derives.  A crossover that moves turns this red instead of quietly testing another kernel.  (Profiling keeps a
    call on one stream; it is not part of the latency / mid-size / throughput predicates.)"""
    lib = engine.load()
    seen = set()
    for (B, N, M), d, kid in FIT64_CASES:
        got = observed_schedule(profiled([ctx64.h], lib, fit_predict_case(ctx64, F64, B, N, d, M, kid)("base"))[0])
        assert got == expected_schedule(True, B, N, d, kid), ("fp64", B, N, M, d, kid, got)
        seen.add(("fp64", got))
    for (B, N, M) in FIT32:
        for d in (1, 3):
            got = observed_schedule(profiled([ctx32.h], lib, fit_predict_case(ctx32, F32, B, N, d, M, 1)("base"))[0])
            assert got == expected_schedule(False, B, N, d, 1), ("fp32", B, N, M, d, got)
            seen.add(("fp32", got))
    for (B, N) in TILED:
        ctx64.joint_reserve(B, 17)
        got = observed_schedule(profiled([ctx64.h], lib, cov_case(ctx64, B, N, 3, 17)("base"))[0])
        assert got == expected_schedule(True, B, N, 3, 1, tiled_only=True), ("cov", B, N, got)
    hs = [lib.cgp_sweep_context(sweep.h, i) for i in range(2)]
    for (B, N, M) in FIT64:
        for d in (1, 3):
            got = [observed_schedule(p) for p in profiled(hs, lib, sweep_case(sweep, B, N, d, M)("base"))]
            sizes = [b - a for a, b in (sweep.shard(B, i) for i in range(2))]
            assert got == [expected_schedule(True, n, N, d, 1, lat_cap=25) for n in sizes], ("sweep", B, N, M, d, got)
            seen.update(("sweep", g) for g in got)
    assert seen >= {("fp64", SMALL), ("fp64", LATENCY), ("fp64", DENSE), ("fp32", LATENCY), ("fp32", DENSE), ("sweep", SMALL),
                    ("sweep", LATENCY)}, seen


def sweep_case(sweep, B, N, d, M):
    cut = [sweep.shard(B, i) for i in range(2)]
    assert cut[0][0] == 0 and cut[0][1] == cut[1][0] and cut[1][1] == B and cut[1][0] < B

    def build(mode):
        X, y, Xs, th = fit_data(B, N, d, M, 1, mode == "fail")
        regs = []
        for i, (a, b) in enumerate(cut):
            t = "@%d" % i
            regs += [IN("dX" + t, F64, X[a:b].transpose(0, 2, 1)), IN("dy" + t, F64, y[a:b]), IN("dXs" + t, F64, Xs[a:b].transpose(0, 2, 1)),
                     IN("dtheta" + t, F64, th[a:b])]
            if mode == "normal":
                regs.append(IN("djitter" + t, F64, 1e-9 * (np.arange(a, b) % 3)))
            regs += [R("dmean" + t, F64, (b - a, M), rowfail=i == 1), R("dvar" + t, F64, (b - a, M), rowfail=i == 1),
                     R("dlogml" + t, F64, (b - a,), rowfail=i == 1), R("dinfo" + t, I32, (b - a,), rowfail=i == 1)]

        def call(p):
            arg = lambda k: [p[k + "@0"], p[k + "@1"]]
            assert sweep.fit_predict_device(B, N, d, M, 1, arg("dX"), arg("dy"), arg("dXs"), arg("dtheta"),
                                            arg("djitter") if mode == "normal" else None, True, arg("dmean"), arg("dvar"),
                                            arg("dlogml"), arg("dinfo"), None) == 0
        return Case(regs, call, zero=("dinfo@0", "dinfo@1"), nonzero_on_fail=("dinfo@1",), sync=sweep.synchronize)
    return build


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("shape", FIT64, ids=ids)
def test_sweep_fit_predict_device(sweep, shape, d):
    """Two contexts on device 0, the batch cut into two contiguous shards with buffers of their own; the failing fit is the last
    of the last shard."""
    B, N, M = shape
    check_case(sweep_case(sweep, B, N, d, M))


# ---- joint forecast after fits ---------------------------------------------------------------------------------------------------
TILED = [(3, 129), (3, 257), (49, 161)]


def joint_d(M):
    """d rides on M on purpose (d = 1 at M = 17, d = 3 at M = 1 and 33): both values are seen by every joint entry point without
    doubling the matrix; the marginal fits above cross d with every shape."""
    return 1 if M == 17 else 3


def cov_case(ctx64, B, N, d, M):
    def build(mode):
        regs = fit_regions(F64, B, N, d, M, 1, mode) + [R("dmean", F64, (B, M)), R("dcov", F64, (B, M, M), nan=True),
                                                        R("dlogml", F64, (B,)), R("dinfo", I32, (B,))]

        def call(p):
            assert ctx64.fit_predict_cov_batch_device(B, N, d, M, 1, p["dX"], p["dy"], p["dXs"], p["dtheta"], jit(p), True, p["dmean"],
                                                      p["dcov"], p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    return build


@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("BN", TILED, ids=ids)
def test_fit_predict_cov_batch_device(ctx64, BN, M):
    (B, N), d = BN, joint_d(M)
    ctx64.joint_reserve(B, M)      # exactly the call's size: the scratch is mpad x mpad per fit, the caller's dcov M x M
    check_case(cov_case(ctx64, B, N, d, M))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("BN", TILED, ids=ids)
def test_fit_sample_batch_device(ctx64, BN, M, S):
    (B, N), d = BN, joint_d(M)
    ctx64.joint_reserve(B, M)
    xi = np.random.default_rng(100 * M + S).normal(size=(B, S, M))

    def build(mode):
        regs = fit_regions(F64, B, N, d, M, 1, mode) + [IN("dxi", F64, xi), R("dout", F64, (B, S, M), nan=True), R("dlogml", F64, (B,)),
                                                        R("dinfo", I32, (B,)), R("dsinfo", I32, (B,), optional=True)]

        def call(p):
            assert ctx64.fit_sample_batch_device(B, N, d, M, 1, p["dX"], p["dy"], p["dXs"], p["dtheta"], jit(p), True, S, p["dxi"], 1e-6,
                                                 p["dout"], p["dlogml"], p["dinfo"], p["dsinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo", "dsinfo"), nonzero_on_fail=("dinfo", "dsinfo"))
    check_case(build)


# ---- multi-target fits -----------------------------------------------------------------------------------------------------------
MULTI = [(2, 129, 17), (3, 257, 33)]
PS = [1, 3, 65, 129]


def targets(y, P):
    """Y (B, P, N): column 0 is y, the others y plus seeded noise of its own scale."""
    rng = np.random.default_rng(P)
    Y = y[:, None, :] + 0.02 * rng.normal(size=(y.shape[0], P, y.shape[1]))
    Y[:, 0] = y
    return Y


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", MULTI, ids=ids)
def test_fit_predict_multi_batch_device(ctx64, shape, P, rows):
    (B, N, M), d = shape, 3
    ctx64.multi_reserve(B, P)      # exactly (B, P): Z is padded to 128 targets inside, the caller's arrays are not

    def build(mode):
        regs = fit_regions(F64, B, N, d, M, 1, mode)
        regs[1] = IN("dY", F64, targets(regs[1].data, P))
        regs += [R("dmean", F64, (B, P, M), nan=True), R("dvar", F64, (B, M), nan=True), R("dlogml", F64, (B, P), nan=True),
                 R("dinfo", I32, (B,))]

        def call(p):
            ctx64.multi_set_form(rows)
            try:
                assert ctx64.fit_predict_multi_batch_device(B, N, d, M, P, 1, p["dX"], p["dY"], p["dXs"], p["dtheta"], jit(p), True,
                                                            p["dmean"], p["dvar"], p["dlogml"], p["dinfo"], 0) == 0
            finally:
                ctx64.multi_set_form(0)
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", MULTI, ids=ids)
def test_multi_nll_grad_batch_device(ctx64, shape, P, extra):
    (B, N, _), d = shape, 3
    nth, stride = d + 2, d + 2 + extra
    ctx64.multi_reserve(B, P)
    ctx64.multi_grad_reserve(B, P)

    def build(mode):
        regs = fit_regions(F64, B, N, d, 1, 1, mode)
        regs[1] = IN("dY", F64, targets(regs[1].data, P))
        del regs[2]                # no test points
        regs += [R("dnll", F64, (B,), nan=True), R("dgrad", F64, (B, stride), keep=np.arange(stride) >= nth, nan=True),
                 R("dlogml", F64, (B, P), optional=True, nan=True), R("dinfo", I32, (B,))]

        def call(p):
            assert ctx64.multi_nll_grad_batch_device(B, N, d, P, 1, p["dX"], p["dY"], p["dtheta"], jit(p), p["dnll"], p["dgrad"], stride,
                                                     p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)


# ---- leave-one-out ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("BN", [(3, 15), (3, 129), (2, 257)], ids=ids)
def test_loo_batch_device(ctx64, BN, d):
    B, N = BN

    def build(mode):
        regs = fit_regions(F64, B, N, d, 1, 1, mode)
        del regs[2]
        regs += [R(k, F64, (B, N), optional=True, nan=True) for k in ("dloo_mean", "dloo_var", "dloo_lpd")]
        regs += [R("dlpd_sum", F64, (B,), optional=True, nan=True), R("dlogml", F64, (B,)), R("dinfo", I32, (B,))]

        def call(p):
            assert ctx64.loo_batch_device(B, N, d, 1, p["dX"], p["dy"], p["dtheta"], jit(p), p["dloo_mean"], p["dloo_var"], p["dloo_lpd"],
                                          p["dlpd_sum"], p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)


# ---- resident windows ------------------------------------------------------------------------------------------------------------
WIN = [(W, N, d) for W in (1, 3) for N in (17, 33, 130) for d in (1, 2)]
STATES = ["filling", "wrapped"]
WKID = 1


def pre_ticks(N, state):
    """Ticks pushed before the call under test: half a window (still filling after the longest push of 5), two windows and three
    ticks (full, slid and moved back to the ring's origin once), two short of the tick that moves the ring (a push across it)."""
    return {"filling": N // 2, "wrapped": 2 * N + 3, "compacting": 2 * N - 2}[state]


@functools.lru_cache(maxsize=None)
def win_data(W, N, d):
    """Streams of 2 N + 48 ticks per window, hyper-parameters of its own for every window."""
    T = 2 * N + 48
    rng = np.random.default_rng(500 + 10 * N + d)
    t = np.arange(11, 11 + T, dtype=np.float64)
    X = np.empty((W, T, d))
    X[:, :, 0] = (t - t.mean()) / t.std() * rng.uniform(0.8, 1.25, (W, 1))
    X[:, :, 1:] = rng.normal(size=(W, T, d - 1))
    y = np.stack([synth._slip_series(rng, t) for _ in range(W)])
    theta = np.column_stack([rng.uniform(0.01, 0.04, W), rng.uniform(0.8, 1.6, (W, d)), rng.uniform(0.5e-3, 2e-3, W)])
    return X, y, theta


def other_theta(theta):
    return theta * np.linspace(1.2, 0.8, theta.shape[1])[None, :]


def win_setup(ctx, W, N, d, state, fail=False, reserve=0):
    """The resident state every run of a case starts from: init, `pre` ticks through the host push, the joint reservation at
    exactly M, and for the failure runs the LAST window failed by cgp_window_set_theta_device (sigma_n^2 = -2 sigma_f^2)."""
    X, y, theta = win_data(W, N, d)
    pre = pre_ticks(N, state)
    ctx.window_init(W, N, d, WKID, theta)
    ctx.window_push(X[:, :pre], y[:, :pre])
    if reserve:
        ctx.window_joint_reserve(reserve)
    if fail:
        bad = theta.copy()
        bad[-1, -1] = -2.0 * bad[-1, 0]
        dth = torch.from_numpy(bad).to(DEV)
        dsel = torch.tensor([0] * (W - 1) + [1], dtype=U8, device=DEV)
        di = torch.zeros(W, dtype=I32, device=DEV)
        torch.cuda.synchronize()
        assert ctx.window_set_theta_device(dth.data_ptr(), d + 2, dsel.data_ptr(), 0, di.data_ptr(), 0) == 0
        torch.cuda.synchronize()
        assert di[-1].item() != 0 and not di[:-1].any()
    return X, y, theta, pre


def test_window_push_cases_reach_both_reachable_kernels(engine, wctx):
    """The launch plans of the push cases below, from cgp_debug_window_plan: at one and three windows a push is cut into
    k_window_ticks (filling, single and left-over ticks, the tick that moves the ring) and k_window_pairs with one window per
    workgroup (pairs of steady-state ticks).  Not reachable at these sizes: k_window_pairs with two or four windows per workgroup
    (from 1 024 windows) and k_window_multi<4> (from 512 windows); tests/test_gpu_window_paths.py runs those."""
    kinds = {}
    for (W, N, d) in WIN:
        for state in STATES + ["compacting"]:
            win_setup(wctx, W, N, d, state)
            for T in (1, 3, 5):
                plan = wctx.window_plan(T)
                assert sum(q[3] for q in plan) == T and all(q[0] in (engine.PLAN_TICKS, engine.PLAN_PAIRS) for q in plan), plan
                assert all(q[1] == 1 for q in plan if q[0] == engine.PLAN_PAIRS), plan
                kinds.setdefault((state, T), set()).update(q[0] for q in plan)
    assert all(kinds[("filling", T)] == {engine.PLAN_TICKS} for T in (1, 3, 5)), kinds
    assert kinds[("wrapped", 1)] == {engine.PLAN_TICKS} and engine.PLAN_PAIRS in kinds[("wrapped", 3)], kinds
    assert kinds[("wrapped", 5)] == {engine.PLAN_TICKS, engine.PLAN_PAIRS}, kinds
    assert engine.PLAN_TICKS in kinds[("compacting", 5)], kinds


@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("state", STATES + ["compacting"])
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_push_device(wctx, wnd, state, T):
    """A push on a window that failed earlier still runs that window's ticks (the header promises no NaN there): its rows are
    only required to stay inside; the neighbours are bitwise those beside a healthy window."""
    W, N, d = wnd

    def build(mode):
        X, y, _, pre = win_data(W, N, d) + (pre_ticks(N, state),)
        regs = [IN("dxs", F64, X[:, pre:pre + T]), IN("dys", F64, y[:, pre:pre + T]), R("dpm", F64, (W, T)), R("dpv", F64, (W, T)),
                R("dlm", F64, (W, T))]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail")
            assert wctx.window_push_device(T, p["dxs"], p["dys"], True, p["dpm"], p["dpv"], p["dlm"], 0) == 0
        return Case(regs, call)
    check_case(build)


def forecast_points(W, N, d, state, M):
    X, _, _ = win_data(W, N, d)
    pre = pre_ticks(N, state)
    return X[:, pre:pre + M] + 0.01


@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_predict_device(wctx, wnd, state, M):
    W, N, d = wnd

    def build(mode):
        regs = [IN("dxs", F64, forecast_points(W, N, d, state, M)), R("dmean", F64, (W, M), nan=True), R("dvar", F64, (W, M), nan=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail")
            assert wctx.window_predict_device(M, p["dxs"], True, p["dmean"], p["dvar"], 0) == 0
        return Case(regs, call)
    check_case(build)


@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_predict_cov_device(wctx, wnd, state, M):
    W, N, d = wnd

    def build(mode):
        regs = [IN("dxs", F64, forecast_points(W, N, d, state, M)), R("dmean", F64, (W, M), nan=True), R("dcov", F64, (W, M, M), nan=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail", reserve=M)
            assert wctx.window_predict_cov_device(M, p["dxs"], True, p["dmean"], p["dcov"], 0) == 0
        return Case(regs, call)
    check_case(build)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 17, 33])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_sample_device(wctx, wnd, state, M, S):
    W, N, d = wnd
    xi = np.random.default_rng(10 * M + S).normal(size=(W, S, M))

    def build(mode):
        regs = [IN("dxs", F64, forecast_points(W, N, d, state, M)), IN("dxi", F64, xi), R("dout", F64, (W, S, M), nan=True),
                R("dinfo", I32, (W,), optional=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail", reserve=M)
            assert wctx.window_sample_device(M, p["dxs"], S, p["dxi"], True, 1e-6, p["dout"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_set_theta_device(wctx, wnd, state, extra):
    """theta_stride of ntheta and ntheta + 2 (the gap columns of dtheta hold NaN: an input, and nothing may come of it), a dselect
    with a hole at three windows: the entries of the unselected window keep the prefill, bit for bit."""
    W, N, d = wnd
    nth, stride = d + 2, d + 2 + extra
    select = np.array([1, 0, 1][:W] if W > 1 else [1], dtype=np.uint8)

    def build(mode):
        th = np.full((W, stride), np.nan)
        th[:, :nth] = other_theta(win_data(W, N, d)[2])
        if mode == "fail":
            th[-1, nth - 1] = -2.0 * th[-1, 0]
        regs = [IN("dtheta", F64, th), IN("dselect", U8, select), R("dlogml", F64, (W,), keep=select == 0, optional=True, nan=True),
                R("dinfo", I32, (W,), keep=select == 0, optional=True)]

        def call(p):
            win_setup(wctx, W, N, d, state)
            assert wctx.window_set_theta_device(p["dtheta"], stride, p["dselect"], p["dlogml"], p["dinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    check_case(build)


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_nll_grad_device(wctx, wnd, state, extra):
    W, N, d = wnd
    nth, stride = d + 2, d + 2 + extra

    def build(mode):
        regs = [R("dnll", F64, (W,), nan=True), R("dgrad", F64, (W, stride), keep=np.arange(stride) >= nth, nan=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail")
            assert wctx.window_nll_grad_device(p["dnll"], p["dgrad"], stride, 0) == 0
        return Case(regs, call)
    check_case(build)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("wnd", WIN, ids=ids)
def test_window_loo_device(wctx, wnd, state):
    """Entries [n, N) of a window still filling are NaN as documented -- inside the extent, written by the call (the prefill
    patterns are not that NaN) -- and the guard after the last window's row holds."""
    W, N, d = wnd
    names = ("dloo_mean", "dloo_var", "dloo_lpd")

    def build(mode):
        regs = [R(k, F64, (W, N), optional=True, nan=True) for k in names] + [R("dlpd_sum", F64, (W,), optional=True, nan=True)]

        def call(p):
            win_setup(wctx, W, N, d, state, fail=mode == "fail")
            assert wctx.window_loo_device(p["dloo_mean"], p["dloo_var"], p["dloo_lpd"], p["dlpd_sum"], 0) == 0
        return Case(regs, call)
    check_case(build)
    out = run_slab(build("normal"), 0x3F)
    n = min(N, pre_ticks(N, state))
    for k in names:
        assert torch.isnan(out[k][:, n:]).all() and not torch.isnan(out[k][:, :n]).any(), k
    assert not torch.isnan(out["dlpd_sum"]).any()
