"""The device entry point of the sparse fits with P target columns (cgp_fit_predict_sparse_multi_batch_device) on guard-band
allocations (tests/guarded.py), in test_gpu_sparse_extents.py's pattern and held to the same extent contract: nothing outside the
documented extents is written (guards, inputs), every documented element of every output is written -- dmean (batch, P, M), dvar
(batch, M), dlogml (batch, P), dinfo (batch) --, and no result moves with what lies behind an input or with the element alignment
of the arguments.  The shapes sit off every padding: m + P off the 16-row tiles, P off the 8-column passes, M off the 16-column
tiles, N off the sub-panels."""
import numpy as np
import pytest

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


def run(engine, ctx, arrays, shape, kid, guard_byte, misalign, slab=True):
    """One call with every argument carved out of ONE allocation (slab) or in tensors of their own -> the four outputs."""
    import torch
    from guarded import Slab
    B, N, d, M, m, P = shape
    ins = dict(zip(("X", "Y", "Z", "Xs", "theta"), arrays))
    outs = {"mean": (torch.float64, (B, P, M)), "var": (torch.float64, (B, M)), "logml": (torch.float64, (B, P)), "info": (torch.int32, (B,))}
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
    assert ctx.fit_predict_sparse_multi_batch_device(B, N, d, M, P, m, kid, ptr("X"), ptr("Y"), ptr("Z"), ptr("Xs"), ptr("theta"), 0, True,
                                                     ptr("mean"), ptr("var"), ptr("logml"), ptr("info")) == 0
    torch.cuda.synchronize()
    if slab:
        assert S.check(snap) == [], S.check(snap)
    res = {k: t[k].cpu().numpy().copy() for k in outs}
    if slab:   # every documented element of every output was written: none still holds the prefill pattern
        for k, v in res.items():
            assert not np.any(np.all(v.view(np.uint8).reshape(v.size, -1) == PREFILL, axis=1)), k
    return res


@pytest.mark.parametrize("shape,kid", tm.EXTENT_CASES)
def test_sparse_multi_device_extents(engine, shape, kid):
    B, N, d, M, m, P = shape
    X, Y, Z, Xs, theta = tm.problem(*tm.extent_args(shape, kid))
    th = np.zeros((B, MAXT))
    th[:, :theta.shape[1]] = theta
    arrays = [np.ascontiguousarray(a) for a in (X.transpose(0, 2, 1), Y, Z.transpose(0, 2, 1), Xs.transpose(0, 2, 1), th)]
    ctx = tm.ctx_for(engine, B, N, d, M, m, P)
    ref = run(engine, ctx, arrays, shape, kid, 0, 0, slab=False)
    assert not ref["info"].any() and np.all(np.isfinite(ref["mean"])) and np.all(ref["var"] > 0) and np.all(np.isfinite(ref["logml"]))
    for guard_byte, misalign in ((0x00, 0), (0xFF, 0), (0x7F, 1), (0xFF, 3)):   # 0xFF / 0x7F bytes: NaN behind every input
        got = run(engine, ctx, arrays, shape, kid, guard_byte, misalign)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (k, guard_byte, misalign)
    tm.close(kid, theta[1], X[1], Y[1], Z[1], Xs[1], ref["mean"][1], ref["var"][1], ref["logml"][1])
