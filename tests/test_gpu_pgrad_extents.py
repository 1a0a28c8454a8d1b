"""The extents of every caller buffer of cgp_fit_predict_grad_batch_device on guard-band allocations (tests/guarded.py), with the
machinery and the data of test_gpu_device_extents.py (its module docstring states the four properties a .. d).  The kernels
behind the call work in tiles of 128 extra rows, blocks of 16 samples and 64 test points per workgroup of the contraction, while
ddmean / ddvar are exactly (batch, M, d): nothing outside them is written, every element of them is written, from the arguments
only; either gradient may be NULL; the failing last fit has NaN in its own rows of both and leaves its neighbours' bits alone."""
import pytest
import torch

import test_gpu_device_extents as ex

pytestmark = pytest.mark.gpu
F64, I32 = torch.float64, torch.int32


@pytest.fixture(scope="module")
def ctx(ex_engine):
    c = ex_engine.Context(max_n=257, max_m=130, max_d=3, max_batch=49)
    assert c.pgrad_reserve(49, 130) == 0
    yield c
    c.close()


@pytest.fixture(scope="module")
def ex_engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def pgrad_case(ctx, B, N, d, M, kid):
    def build(mode):
        regs = ex.fit_regions(F64, B, N, d, M, kid, mode) + [
            ex.R("dmean", F64, (B, M)), ex.R("dvar", F64, (B, M)), ex.R("dlogml", F64, (B,)), ex.R("dinfo", I32, (B,)),
            ex.R("ddmean", F64, (B, M, d), optional=True, nan=True), ex.R("ddvar", F64, (B, M, d), optional=True, nan=True)]

        def call(p):
            assert ctx.fit_predict_grad_batch_device(B, N, d, M, kid, p["dX"], p["dy"], p["dXs"], p["dtheta"], ex.jit(p), True,
                                                     p["dmean"], p["dvar"], p["dlogml"], p["dinfo"], p["ddmean"], p["ddvar"], 0) == 0
        return ex.Case(regs, call, zero=("dinfo",), nonzero_on_fail=("dinfo",))
    return build


# (fits, N, M): one block step with a short last 16-block; two steps, one row into the second tile; three steps with M + 1
# above a 128-row tile; one past the latency and mid-size schedules.  SE-ARD at d = 1 and 3, RBF x Brownian and Matern 5/2.
CASES = [((3, 15, 20), 1, 1), ((3, 15, 20), 3, 1), ((3, 129, 17), 3, 1), ((3, 257, 130), 1, 1), ((3, 257, 130), 3, 1),
         ((49, 161, 33), 3, 1), ((3, 161, 17), 1, 2), ((3, 129, 17), 3, 4)]


@pytest.mark.parametrize("shape,d,kid", CASES, ids=ex.ids)
def test_fit_predict_grad_batch_device(ctx, shape, d, kid):
    B, N, M = shape
    ex.check_case(pgrad_case(ctx, B, N, d, M, kid))
