#!/usr/bin/env python3
"""Randomised sweep of the sparse fits' objective with P target columns (cgp_sparse_multi_nll_grad_batch) against
tests/sparse_multi_grad_oracle.py (test infrastructure: uses oracle/): fuzz_sparse_grad.py's generator -- random kernel (all
five), history length, inducing inputs, input dimension, batch, with and without gradZ -- with a random column count P <= 64
(around the 16-row tiles of the augmented panel and the 8-column passes of the column solves) on test_gpu_sparse_multi.py's target
columns.  nll, grad and gradZ are compared with the one-factor statement, the columns' bounds bitwise with the multi-column
forward call, and a P = 1 call on the last column bitwise with the single-column gradient call.  fuzz_sparse_grad.py's conditions
and rejection rule (fuzz_sparse_multi.py's cap: the sweep fails when more than 10 % of the draws are rejected).
   python tests/fuzz/fuzz_sparse_multi_grad.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "tests", "fuzz"))
import numpy as np
import sparse_multi_grad_oracle as smg
import test_gpu_sparse_grad as tgg
import test_gpu_sparse_multi as tm
import fuzz_sparse_grad as fg

PS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64]


def draw(rng):
    c = fg.draw(rng)
    c["P"] = int(rng.choice(PS))
    c["Y"] = tm.add_columns(c["X"], c["theta"], c["kid"], c["P"], c["seed"])
    return c


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
        ok, check = fg.accept(c)   # (the conditions are functions of (X, Z, theta) alone)
        if not ok:
            rejected += 1
            continue
        cases += 1
        ref = [(b, smg.one_factor(c["kid"], c["theta"][b], c["X"][b], c["Y"][b], c["Z"][b])) for b in check]
        if oracle_only:
            continue
        tag = " ".join(f"{k}={c[k]}" for k in ("N", "m", "P", "d", "kid", "B", "with_z", "seed"))
        ctx = engine.Context(max_n=16, max_m=8, max_d=c["d"], max_batch=c["B"])
        ctx.sparse_reserve(c["B"], c["N"], c["m"], 0)
        ctx.sparse_grad_reserve(c["B"])
        ctx.sparse_multi_reserve(c["B"], c["P"])
        ctx.sparse_multi_grad_reserve(c["B"], c["P"])
        rc, nll, g, gz, logml, info = ctx.sparse_multi_nll_grad_batch(c["X"], c["Y"], c["Z"], c["theta"], c["kid"], want_grad_z=c["with_z"])
        rcf, _, _, bound, infof = ctx.fit_predict_sparse_multi_batch(c["X"], c["Y"], c["Z"], None, c["theta"], c["kid"])
        if not (rcf == rc and np.array_equal(bound, logml) and np.array_equal(infof, info)):
            print("FAIL", tag, "the columns' bounds are not bitwise the forward call's"); bad += 1
        last = c["Y"][:, c["P"] - 1]
        one = ctx.sparse_multi_nll_grad_batch(c["X"], last[:, None], c["Z"], c["theta"], c["kid"], want_grad_z=c["with_z"])
        single = ctx.sparse_nll_grad_batch(c["X"], last, c["Z"], c["theta"], c["kid"], want_grad_z=c["with_z"])
        same = one[0] == single[0] and np.array_equal(one[1], single[1]) and np.array_equal(one[2], single[2]) and \
            (not c["with_z"] or np.array_equal(one[3], single[3]))
        if not same:
            print("FAIL", tag, "P = 1 is not bitwise the single-column call"); bad += 1
        for b, (onll, og, ogz, ologml, oinfo) in ref:
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
