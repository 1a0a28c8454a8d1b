"""The device entry point of the sparse fits' objective with P target columns (cgp_sparse_multi_nll_grad_batch_device) on
guard-band allocations (tests/guarded.py), in test_gpu_sparse_grad_extents.py's pattern and held to the same extent contract: nothing
outside the documented extents is written (guards, inputs), every documented element of every output is written -- dnll (batch),
dgrad's first ntheta entries per fit (the rest of a row of grad_stride > ntheta is not touched), dgradZ (batch, d, m), dlogml
(batch, P), dinfo (batch) --, and no result moves with what lies behind an input or with the element alignment of the arguments.
With and without dgradZ and dlogml, at test_gpu_sparse_multi.EXTENT_CASES."""
import numpy as np
import pytest

import test_gpu_sparse_multi_grad as tmg
import test_gpu_sparse_multi as tm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXT = 10   # CGP_MAX_THETA
PREFILL = 0xA5


@pytest.fixture(scope="module")
def engine():
    import corenav_gp_amd.engine as e
    e.load()
    return e


def run(engine, ctx, arrays, shape, kid, nth, with_z, with_l, guard_byte, misalign, slab=True):
    """One call with every argument carved out of ONE allocation (slab) or in tensors of their own -> the outputs."""
    import torch
    from guarded import Slab
    B, N, d, m, P = shape
    ins = dict(zip(("X", "Y", "Z", "theta"), arrays))
    outs = {"nll": (torch.float64, (B,)), "grad": (torch.float64, (B, MAXT)), "info": (torch.int32, (B,))}
    if with_z:
        outs["gradZ"] = (torch.float64, (B, d, m))
    if with_l:
        outs["logml"] = (torch.float64, (B, P))
    if not slab:
        t = {k: torch.from_numpy(v).to(DEV) for k, v in ins.items()}
        t.update({k: torch.empty(s, dtype=dt, device=DEV) for k, (dt, s) in outs.items()})
        ptr = lambda k: t[k].data_ptr()
    else:
        S = Slab(DEV)
        for k, v in ins.items():
            S.region(k, torch.float64, v.shape, misalign=misalign, role="input")
        for k, (dt, s) in outs.items():
            S.region(k, dt, s, misalign=misalign, role="output")
        S.fill_guards(guard_byte)
        for k, v in ins.items():
            S.view(k).copy_(torch.from_numpy(v))
        for k in outs:
            S.fill(k, PREFILL)
        t = {k: S.view(k) for k in list(ins) + list(outs)}
        ptr = S.ptr
        snap = S.snapshot()
    assert ctx.sparse_multi_nll_grad_batch_device(B, N, d, P, m, kid, ptr("X"), ptr("Y"), ptr("Z"), ptr("theta"), 0, ptr("nll"),
                                                  ptr("grad"), MAXT, ptr("gradZ") if with_z else 0, ptr("logml") if with_l else 0,
                                                  ptr("info")) == 0
    torch.cuda.synchronize()
    if slab:
        assert S.check(snap) == [], S.check(snap)
    res = {k: t[k].cpu().numpy().copy() for k in outs}
    if slab:   # every documented element was written, and the tail of a grad row was not
        untouched = lambda v: np.all(v.view(np.uint8).reshape(v.size, -1) == PREFILL, axis=1)
        assert np.all(untouched(np.ascontiguousarray(res["grad"][:, nth:])))
        res["grad"] = np.ascontiguousarray(res["grad"][:, :nth])
        for k, v in res.items():
            assert not np.any(untouched(v)), k
    else:
        res["grad"] = np.ascontiguousarray(res["grad"][:, :nth])
    return res


@pytest.mark.parametrize("with_z,with_l", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("shape,kid", tm.EXTENT_CASES)
def test_sparse_multi_grad_device_extents(engine, shape, kid, with_z, with_l):
    B, N, d, M, m, P = shape
    X, Y, Z, theta = tmg.extent(shape, kid)
    nth = theta.shape[1]
    assert nth < MAXT
    th = np.zeros((B, MAXT))
    th[:, :nth] = theta
    arrays = [np.ascontiguousarray(a) for a in (X.transpose(0, 2, 1), Y, Z.transpose(0, 2, 1), th)]
    ctx = tmg.ctx_for(engine, B, N, d, m, P)
    ref = run(engine, ctx, arrays, (B, N, d, m, P), kid, nth, with_z, with_l, 0, 0, slab=False)
    assert not ref["info"].any() and all(np.all(np.isfinite(v)) for v in ref.values())
    for guard_byte, misalign in ((0x00, 0), (0xFF, 0), (0x7F, 1), (0xFF, 3)):   # 0xFF / 0x7F bytes: NaN behind every input
        got = run(engine, ctx, arrays, (B, N, d, m, P), kid, nth, with_z, with_l, guard_byte, misalign)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (k, guard_byte, misalign)
    gz = ref["gradZ"][1].T if with_z else None
    tmg.close(kid, theta[1], X[1], Y[1], Z[1], ref["nll"][1], ref["grad"][1], gz, ref["logml"][1] if with_l else None)
