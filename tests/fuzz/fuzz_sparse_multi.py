#!/usr/bin/env python3
"""Randomised sweep of the sparse fits with P target columns (cgp_fit_predict_sparse_multi_batch) against
tests/sparse_multi_oracle.py (test infrastructure: uses oracle/): fuzz_sparse.py's generator -- random kernel (all five), history
length, inducing inputs, input dimension, test points (0 among them), batch, noise on / off -- with a random column count P <= 64
(around the 16-row tiles of the augmented matrix and the 8-column passes of the column solves) on test_gpu_sparse_multi.py's target
columns.  Every column is compared with the one-factor statement, columns 0, P // 2 and P - 1 with the per-column definition, and
column P - 1 bitwise with the single-column call.  fuzz_sparse.py's conditions and rejection rule.
   python tests/fuzz/fuzz_sparse_multi.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "tests", "fuzz"))
import numpy as np
import sparse_multi_oracle as smo
import test_gpu_sparse_multi as tm
import fuzz_sparse as fs

PS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64]


def draw(rng):
    c = fs.draw(rng)
    c["P"] = int(rng.choice(PS))
    c["Y"] = tm.add_columns(c["X"], c["theta"], c["kid"], c["P"], c["seed"])
    return c


def accept(c):
    """(every checked fit meets the oracle's conditions, both statements of the fits that are checked: the first and the last)."""
    ref = []
    for b in sorted({0, c["B"] - 1}):
        xs = c["Xs"][b] if c["M"] else None
        o = smo.per_column(c["kid"], c["theta"][b], c["X"][b], c["Y"][b], c["Z"][b], xs, c["noise"], cols=tm.oracle_columns(c["P"]))
        if not (o.info == 0 and o.ladder == 0 and o.cond_uu <= 1e6 and o.cond_b <= 1e8):
            return False, []
        ref.append((b, o, smo.one_factor(c["kid"], c["theta"][b], c["X"][b], c["Y"][b], c["Z"][b], xs, c["noise"])))
    return True, ref


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
        ok, ref = accept(c)
        if not ok:
            rejected += 1
            continue
        cases += 1
        if oracle_only:
            continue
        tag = " ".join(f"{k}={c[k]}" for k in ("N", "m", "P", "d", "kid", "B", "M", "noise", "seed"))
        ctx = engine.Context(max_n=16, max_m=max(c["M"], 8), max_d=c["d"], max_batch=c["B"])
        ctx.sparse_reserve(c["B"], c["N"], c["m"], c["M"])
        ctx.sparse_multi_reserve(c["B"], c["P"])
        xs = c["Xs"] if c["M"] else None
        rc, mean, var, bound, info = ctx.fit_predict_sparse_multi_batch(c["X"], c["Y"], c["Z"], xs, c["theta"], c["kid"], include_noise=c["noise"])
        last = c["P"] - 1
        rc1, m1, v1, b1, i1 = ctx.fit_predict_sparse_batch(c["X"], c["Y"][:, last], c["Z"], xs, c["theta"], c["kid"], include_noise=c["noise"])
        same = (np.array_equal(m1, mean[:, last]) and np.array_equal(b1, bound[:, last]) and np.array_equal(v1, var)
                and np.array_equal(i1, info) and rc1 == rc)
        if not same:
            print("FAIL", tag, "column", last, "is not bitwise the single-column call"); bad += 1
        for b, o, of in ref:
            e = float(max(max(smo.errors(mean[b], var[b], bound[b], r)) for r in (o, of)))
            worst = max(worst, e / 1e-6)
            if not (e < 1e-6) or info[b] != 0 or rc != 0:
                print("FAIL", tag, "fit", b, "err", e, "info", info[b], "rc", rc); bad += 1
        ctx.close()
    share = rejected / max(drawn, 1)
    print(f"draws {drawn} rejected {rejected} ({100.0 * share:.0f} %)")
    print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
    return 1 if bad or share > 0.1 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
