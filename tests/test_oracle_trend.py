"""The yardstick of the trend tests pinned (CPU): tests/trend_oracle.py against 50-digit arithmetic, two ways
(tests/golden/gen_trend_golden.py wrote the pins): the closed form of Rasmussen & Williams 2.7 written with Ky^-1 itself, and the
zero-mean GP with kernel k + b^2 h h'^T at b^2 = 1e12 -- no trend formula at all.  Bar 1e-9 for both, in trend_oracle.errors'
metric; float64 sits at 1e-16 .. 1e-13 against either.  The conditions every compared input must meet -- no jitter, cond(A) <=
1e6, every pivot of A passes the rank rule by a factor of at least 1e3 -- are asserted here, on the pins and on the problems the
GPU tests draw, so that those tests cannot hide behind an ill-conditioned basis."""
import glob
import os

import numpy as np
import pytest

import trend_oracle as to

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PINS = sorted(glob.glob(os.path.join(GOLDEN, "trend_mp_*.npz")))
BAR = 1e-9


def test_the_pins_are_there():
    assert len(PINS) == 3


@pytest.mark.parametrize("path", PINS, ids=[os.path.basename(p)[:-4] for p in PINS])
@pytest.mark.parametrize("tag", ["closed", "limit"])
def test_oracle_against_50_digits(path, tag):
    g = np.load(path)
    o = to.fit_predict_trend(int(g["kid"]), g["theta"], g["X"], g["Y"], g["H"], g["Xs"], g["Hs"], noise=True)
    assert to.conditions_hold(o), (o.tinfo, o.jitter, o.cond, o.margin)
    assert 1.0 <= o.cond <= 100.0
    ref = to.SimpleNamespace(mean=g[tag + "_mean"], var=g[tag + "_var"], beta=g[tag + "_beta"], logml=g[tag + "_logml"])
    e = to.errors(o.mean, o.var, o.beta, o.logml, ref)
    print(f"{os.path.basename(path)} {tag}: cond(A) {o.cond:.3g} margin {o.margin:.3g} errors mean {e[0]:.2e} var {e[1]:.2e} "
          f"beta {e[2]:.2e} logml {e[3]:.2e}")
    assert max(e) <= BAR, e
    assert np.all(o.var - o.base >= 0.0)


def test_rank_rule_of_the_oracle():
    """A duplicated column fails at its own index, a NaN column too, and n < q fails at pivot n + 1 for the tests' basis."""
    rng = np.random.default_rng(0)
    G = rng.normal(size=(20, 3))
    assert to.pivots(G.T @ G)[1] == 0
    G[:, 2] = G[:, 0]
    assert to.pivots(G.T @ G)[1] == 3
    G[:, 1] = np.nan
    assert to.pivots(G.T @ G)[1] == 2
    for n in (0, 1, 2):
        Gn = to.basis(np.array([1.0, 2.5, 4.0])[:n], 2.0, 1.5, 3).T
        assert to.pivots(Gn.T @ Gn)[1] == n + 1


def test_shift_property_of_the_oracle():
    """Y -> Y + H^T c shifts beta by c and the mean by Hs^T c; var and logml do not move (1e-9)."""
    g = np.load(os.path.join(GOLDEN, "trend_mp_se1_q2.npz"))
    kid, th = int(g["kid"]), g["theta"]
    c = np.array([[0.7, -0.3], [2.0, 0.1]])   # (P, q)
    a = to.fit_predict_trend(kid, th, g["X"], g["Y"], g["H"], g["Xs"], g["Hs"])
    b = to.fit_predict_trend(kid, th, g["X"], g["Y"] + c @ g["H"], g["H"], g["Xs"], g["Hs"])
    assert np.max(np.abs(b.beta - a.beta - c)) <= 1e-9 and np.max(np.abs(b.mean - a.mean - c @ g["Hs"])) <= 1e-9
    assert np.array_equal(a.var, b.var) and np.max(np.abs(a.logml - b.logml)) <= 1e-9 * np.max(np.abs(a.logml))


def test_fuzz_generator_rejects_few():
    """tests/fuzz/fuzz_trend.py draws only inputs for which the conditions above hold and counts what it rejects: the generator
    alone (no GPU) stays under 20 %."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
    import fuzz_trend
    rng = np.random.default_rng(2024)
    drawn = rejected = 0
    while drawn - rejected < 12:
        case = fuzz_trend.draw(rng)
        drawn += 1
        rejected += not fuzz_trend.accept(case)[0]
    print(f"fuzz_trend generator: {rejected} of {drawn} draws rejected ({100.0 * rejected / drawn:.0f} %)")
    assert rejected <= 0.2 * drawn
