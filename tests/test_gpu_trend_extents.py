"""The extents of every caller buffer of cgp_fit_predict_trend_batch_device on guard-band allocations (tests/guarded.py), by the
method and with the machinery of tests/test_gpu_device_extents.py (its docstring states what is asserted: nothing outside the
documented extents written, every documented element written, results independent of guard content and of element alignment, a
failed fit beside healthy ones).  The reservations are exactly the call's; P + q sits on both sides of the 16-column chunks of the
Gram kernel and of the 64- and 128-row tiles of the solve, M on both sides of the 128 test points of a k_trend_apply workgroup."""
import numpy as np
import pytest

from test_gpu_device_extents import F64, I32, R, IN, Case, check_case, fit_regions, jit, ids
from test_gpu_device_extents import targets
from test_gpu_trend import basis

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


@pytest.fixture(scope="module")
def ctx64(engine):
    c = engine.Context(max_n=257, max_m=257, max_d=3, max_batch=49)
    yield c
    c.close()


def basis_of(x0, c, s, q):
    return np.stack([basis(x, cc, ss, q) for x, cc, ss in zip(x0, c, s)])      # (B, q, len)


@pytest.mark.parametrize("P,q", [(1, 1), (14, 3), (63, 2), (120, 16)])
@pytest.mark.parametrize("shape", [(2, 129, 17), (3, 257, 130)], ids=ids)
def test_fit_predict_trend_batch_device(ctx64, shape, P, q):
    (B, N, M), d = shape, 3
    ctx64.multi_reserve(B, P + 16)
    ctx64.trend_reserve(B, P, M)      # exactly (B, P, M)

    def build(mode):
        regs = fit_regions(F64, B, N, d, M, 1, mode)
        x0, xs0 = regs[0].data[:, 0, :], regs[2].data[:, 0, :]
        c, s = x0.mean(axis=1), np.maximum(x0.std(axis=1), 1e-3)
        regs[1] = IN("dY", F64, targets(regs[1].data, P))
        regs += [IN("dH", F64, basis_of(x0, c, s, q)), IN("dHs", F64, basis_of(xs0, c, s, q)), R("dmean", F64, (B, P, M), nan=True),
                 R("dvar", F64, (B, M), nan=True), R("dbeta", F64, (B, P, q), nan=True), R("dlogml", F64, (B, P), nan=True),
                 R("dinfo", I32, (B,)), R("dtinfo", I32, (B,), rowfail=False)]

        def call(p):
            assert ctx64.fit_predict_trend_batch_device(B, N, d, M, P, q, 1, p["dX"], p["dY"], p["dH"], p["dXs"], p["dHs"], p["dtheta"],
                                                        jit(p), True, p["dmean"], p["dvar"], p["dbeta"], p["dlogml"], p["dinfo"],
                                                        p["dtinfo"], 0) == 0
        return Case(regs, call, zero=("dinfo", "dtinfo"), nonzero_on_fail=("dinfo",))
    check_case(build)
