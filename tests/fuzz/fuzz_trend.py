#!/usr/bin/env python3
"""Randomised sweep of the explicit-basis (trend) fits (cgp_fit_predict_trend_batch: the multi-target launches on the P + q packed
columns, k_trend_pack, k_trend_gram, k_trend_solve, k_trend_apply) against tests/trend_oracle.py (test infrastructure: uses
oracle/): random kernel (all five), window length N <= 300 (around the 4-, 16- and 128-sample boundaries), input dimension, number
of test points M <= 130, of targets P <= 70 and of basis columns q <= 3 (the basis [1, u, u^2][:q] of the tests), batch <= 3,
noise on / off.  Only inputs that meet the oracle's own conditions are compared (no jitter, cond(A) <= 1e6, every pivot of A
passes the rank rule by 1e3): a draw that does not is REJECTED and counted, and the sweep fails when more than 20 % are.
   python tests/fuzz/fuzz_trend.py [seconds=60] [seed=0] [max_cases=0 (no limit)] [oracle-only]
oracle-only: no GPU -- draws the same cases and runs the oracle alone."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
from corenav_gp_amd import synth
import trend_oracle as to

NS = [3, 4, 5, 15, 16, 17, 63, 65, 100, 127, 128, 129, 134, 200, 255, 256, 257, 300]
MS = [1, 2, 15, 16, 17, 33, 64, 65, 100, 127, 128, 129]
PS = [1, 2, 3, 4, 13, 14, 15, 16, 17, 48, 61, 62, 63, 64, 65, 70]


def draw(rng):
    """One case: a dict of the call's arrays and shape."""
    N, M, P = int(rng.choice(NS)), int(rng.choice(MS)), int(rng.choice(PS))
    q = int(rng.integers(1, 4))
    kid = int(rng.integers(0, 5))
    d = 1 if kid == 2 else int(rng.integers(1, 7))
    B = int(rng.integers(1, 4))
    noise = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 1 << 30))
    Xw, Yw, Xsw, Hw, Hsw = [], [], [], [], []
    for b in range(B):
        r2 = np.random.default_rng(seed + b)
        t = np.arange(11 + b, 11 + b + N, dtype=np.float64)
        Y = np.stack([synth._slip_series(np.random.default_rng(seed + 1000 * (p + 1) + b), t) + 0.1 for p in range(P)])
        X = t[:, None] if d == 1 else np.column_stack([(t - t.mean()) / max(t.std(), 1.0)] + [r2.normal(size=N) for _ in range(d - 1)])
        Xs = X[-1:, :] + 1.0 + np.arange(M, dtype=np.float64)[:, None] if kid == 2 else \
            X[r2.integers(max(0, N - 50), N, size=M)] + 0.3 * r2.normal(size=(M, d))
        c, s = float(X[:, 0].mean()), float(max(X[:, 0].std(), 1e-3))
        Xw.append(X); Yw.append(Y); Xsw.append(Xs); Hw.append(to.basis(X[:, 0], c, s, q)); Hsw.append(to.basis(Xs[:, 0], c, s, q))
    th1 = {2: np.array([0.5, 30.0, 0.01, 0.002]), 0: np.array([0.02, 1.0, 1e-3])}.get(kid, np.concatenate([[0.02], np.linspace(0.8, 1.6, d), [1e-3]]))
    return dict(N=N, M=M, P=P, q=q, kid=kid, d=d, B=B, noise=noise, seed=seed, X=np.stack(Xw), Y=np.stack(Yw), Xs=np.stack(Xsw),
                H=np.stack(Hw), Hs=np.stack(Hsw), theta=np.tile(th1, (B, 1)))


def accept(c):
    """(every checked fit meets the oracle's conditions, the oracle's answers of the fits that are checked: the first and the last)."""
    check = sorted({0, c["B"] - 1})
    ref = [to.fit_predict_trend(c["kid"], c["theta"][b], c["X"][b], c["Y"][b], c["H"][b], c["Xs"][b], c["Hs"][b], c["noise"]) for b in check]
    return all(to.conditions_hold(o) for o in ref), list(zip(check, ref))


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
        tag = " ".join(f"{k}={c[k]}" for k in ("N", "d", "kid", "B", "M", "P", "q", "noise", "seed"))
        ctx = engine.Context(max_n=c["N"], max_m=c["M"], max_d=c["d"], max_batch=c["B"])
        ctx.multi_reserve(c["B"], c["P"] + 16)
        ctx.trend_reserve(c["B"], c["P"], c["M"])
        rc, mean, var, beta, logml, info, tinfo = ctx.fit_predict_trend_batch(c["X"], c["Y"], c["H"], c["Xs"], c["Hs"], c["theta"], c["kid"],
                                                                              include_noise=c["noise"])
        for b, o in ref:
            e = float(max(to.errors(mean[b], var[b], beta[b], logml[b], o)))
            worst = max(worst, e / 1e-6)
            if not (e < 1e-6) or info[b] != 0 or tinfo[b] != 0 or rc != 0:
                print("FAIL", tag, "fit", b, "err", e, "info", info[b], "tinfo", tinfo[b], "rc", rc); bad += 1
        ctx.close()
    share = rejected / max(drawn, 1)
    print(f"draws {drawn} rejected {rejected} ({100.0 * share:.0f} %)")
    print(f"cases {cases} failures {bad} worst error / bar {worst:.3g}")
    return 1 if bad or share > 0.2 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
