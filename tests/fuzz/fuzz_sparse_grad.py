#!/usr/bin/env python3
"""Randomised sweep of the sparse fits' objective (cgp_sparse_nll_grad_batch: the forward chain, k_sparse_grad_algebra,
k_sparse_grad_panel, k_sparse_grad_uu, k_sparse_grad_finish) against tests/sparse_grad_oracle.py (test infrastructure: uses
oracle/): random kernel (all five), history length N <= 1100 (around the sub-panel and chunk boundaries), inducing inputs m <= 200
(around the 16-row tiles and the groups of eight row tiles), input dimension, batch <= 3, with and without gradZ, on the lattice
problems of tests/test_gpu_sparse.py.  Only inputs that meet the oracle's own conditions are compared (no ladder step, cond(K_uu)
<= 1e6, cond(B) <= 1e8): a draw that does not is REJECTED and counted, and the sweep fails when more than 10 % are.
   python tests/fuzz/fuzz_sparse_grad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
oracle-only: no GPU -- draws the same cases and runs the oracle alone."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import sparse_oracle as so
import sparse_grad_oracle as sg
import test_gpu_sparse as tg
import test_gpu_sparse_grad as tgg

NS = [1, 2, 7, 8, 9, 15, 16, 17, 63, 65, 130, 257, 511, 512, 513, 1024, 1027, 1100]
MI = [1, 2, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 144, 145, 200]


def draw(rng):
    """One case: a dict of the call's arrays and shape."""
    N, m = int(rng.choice(NS)), int(rng.choice(MI))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 5))
    B = int(rng.integers(1, 4))
    with_z = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1 << 30))
    X, y, Z, _, theta = tg.problem(B, N, d, 0, m, kid, seed)
    return dict(N=N, m=m, kid=kid, d=d, B=B, with_z=with_z, seed=seed, X=X, y=y, Z=Z, theta=theta)


def accept(c):
    """(every checked fit meets the oracle's conditions, the fits that are checked: the first and the last)."""
    check = sorted({0, c["B"] - 1})
    return all(so.conditions_hold(so.fit_predict_sparse(c["kid"], c["theta"][b], c["X"][b], c["y"][b], c["Z"][b], None)) for b in check), check


def main(argv):
    oracle_only = "oracle-only" in argv
    argv = [a for a in argv if a != "oracle-only"]
    if not oracle_only:
        import torch  # noqa: F401
        from corenav_gp_amd import engine
    budget = float(argv[0]) if len(argv) > 0 else 60.0
    rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
    max_cases = int(argv[2]) if len(argv) > 2 else 0
    t_end, cases, drawn, rejected, bad, worst = time.time() + budget, 0, 0, 0, 0, 0.0
    while time.time() < t_end and (max_cases == 0 or cases < max_cases):
        c = draw(rng)
        drawn += 1
        ok, check = accept(c)
        if not ok:
            rejected += 1
            continue
        cases += 1
        ref = [(b, sg.nll_grad(c["kid"], c["theta"][b], c["X"][b], c["y"][b], c["Z"][b])) for b in check]
        if oracle_only:
            continue
        tag = " ".join(f"{k}={c[k]}" for k in ("N", "m", "d", "kid", "B", "with_z", "seed"))
        ctx = engine.Context(max_n=16, max_m=8, max_d=c["d"], max_batch=c["B"])
        ctx.sparse_reserve(c["B"], c["N"], c["m"], 0)
        ctx.sparse_grad_reserve(c["B"])
        rc, nll, g, gz, info = ctx.sparse_nll_grad_batch(c["X"], c["y"], c["Z"], c["theta"], c["kid"], want_grad_z=c["with_z"])
        for b, (onll, og, ogz, oinfo) in ref:
            e = float(max(tgg.errors(nll[b], g[b], gz[b] if c["with_z"] else None, onll, og, ogz)))
            worst = max(worst, e / 1e-6)
            if not (e < 1e-6) or info[b] != 0 or rc != 0 or oinfo != 0:
                print("FAIL", tag, "fit", b, "err", e, "info", info[b], "rc", rc); bad += 1
        ctx.close()
    share = rejected / max(drawn, 1)
    print(f"draws {drawn} rejected {rejected} ({100.0 * share:.0f} %)")
    print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
    return 1 if bad or share > 0.1 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
