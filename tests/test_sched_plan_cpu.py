"""Which schedule a fit call takes, checked without a GPU: sched_plan (corenav_gp_amd/csrc/cgp_sched_plan.hpp) is plain host
code, so tests/sched_plan_table.cpp -- a stand-alone program that includes that header and nothing else -- is built with g++
and asked for the plan of every input below.  The expected rows are written out by hand from the predicates and constants of
run_schedule as it stood before the plan existed (either side of every crossover), not produced by the code under test.

A row: (input words, schedule, mid, split_diag, xsplit, use_acc, fits per stream group[, tune, trmm, alpha, refine]) with
refine = "steps,solve,alpha of every fit".  Inputs a call cannot have are there because the predicate names them: ET = 0
(ET = ceil((M + 1) / 128) is at least 1 in every call)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corenav_gp_amd", "csrc")

# contexts whose capacities never bind (cgp_create_ex of a large max_batch), so that the limits seen are the crossovers'
F64 = "esz=8 lat_cap=48 mid_cap=96 lat_units=100000 lat_img_fits=28 M=5 ET=1"
F32 = "esz=4 lat_cap=48 mid_cap=96 lat_units=100000 lat_img_fits=24 M=5 ET=1 refine_bufs=1 refine_max_nt=100"
THR = "no_latency=1"                        # CGP_SCHED=throughput
SPLITDIAG = "no_latency=1 sw_split_diag=1"   # CGP_SCHED=splitdiag
FUSEDDIAG = "no_latency=1 fused_diag=1"      # CGP_SCHED=fuseddiag
OVERLAP = "no_latency=1 overlap=1"           # CGP_SCHED=overlap
ONE = "one_launch=1"                         # CGP_SCHED=onelaunch


def R(words, sched, mid, split_diag, xsplit, acc, gb, tune=0, trmm=1, alpha=0, refine="0,0,0"):
    gb = gb if isinstance(gb, tuple) else (gb,)
    return words, (f"{sched} mid={mid} split_diag={split_diag} xsplit={xsplit} acc={acc} trmm={trmm} tune={tune} G={len(gb)} "
                   f"gb={','.join(map(str, gb))} alpha={alpha} refine={refine}")


def lat64(NT, fits):   # fp64: the largest latency call of NT block steps and the call one fit above it (always mid-size or, at 49, not)
    acc = 1 if NT >= 2 else 0
    return [R(f"{F64} NT={NT} batch={fits}", "Latency", 1, 0, 0, 0, fits),
            R(f"{F64} NT={NT} batch={fits + 1}", "Launches", 1 if fits + 1 <= 48 else 0, 0, 0, acc, fits + 1)]


def lat32(NT, fits):   # fp32 likewise (every such call is mid-size; one refinement step up to eight block steps, two beyond)
    ref = "2,1,0" if NT > 8 else "1,1,0"
    return [R(f"{F32} NT={NT} batch={fits}", "Latency", 1, 0, 0, 0, fits, refine=ref),
            R(f"{F32} NT={NT} batch={fits + 1}", "Launches", 1, 0, 0, 1 if NT >= 2 else 0, fits + 1, refine=ref)]


# rows both libraries answer alike (no measurement switch or override in them)
COMMON = (
    # fp64 latency limits: 48 fits at NT 1 and 2, 28 at 3-4, 22 at 5-6, 18 at 7-8, 13 at 9-12, 11 above
    lat64(1, 48) + lat64(2, 48) + lat64(3, 28) + lat64(4, 28) + lat64(5, 22) + lat64(6, 22) + lat64(7, 18) + lat64(8, 18)
    + lat64(9, 13) + lat64(12, 13) + lat64(13, 11) + lat64(16, 11)
    # fp32 latency limits: 32 fits at NT <= 2, 24 at 3-4, 20 above
    + lat32(1, 32) + lat32(2, 32) + lat32(3, 24) + lat32(4, 24) + lat32(5, 20) + lat32(16, 20)
    + [
        # mid-size limits.  fp64: 48 fits below six block steps, 64 at 6-7, 96 from 8 (where 96 x 8 >= 480 also splits the extra rows off)
        R(f"{F64} NT=5 batch=48", "Launches", 1, 0, 0, 1, 48),
        R(f"{F64} NT=5 batch=49", "Launches", 0, 0, 0, 1, 49),
        R(f"{F64} NT=6 batch=64", "Launches", 1, 0, 0, 1, 64),
        R(f"{F64} NT=6 batch=65", "Launches", 0, 0, 0, 1, 65),
        R(f"{F64} NT=7 batch=64", "Launches", 1, 0, 0, 1, 64),
        R(f"{F64} NT=7 batch=65", "Launches", 0, 0, 0, 1, 65),
        R(f"{F64} NT=8 batch=96", "Launches", 1, 0, 1, 1, 96),
        R(f"{F64} NT=8 batch=97", "Launches", 0, 0, 0, 1, 97),
        # fp32: 96 fits (two stream groups there, the tuner asked; one group above)
        R(f"{F32} NT=8 batch=96", "Launches", 1, 0, 0, 1, (48, 48), tune=1, refine="1,1,0"),
        R(f"{F32} NT=8 batch=97", "Launches", 0, 0, 0, 1, 97, refine="1,1,0"),
        # fp64 split diagonal from 512 fits
        R(f"{F64} NT=3 batch=511", "Launches", 0, 0, 0, 1, 511),
        R(f"{F64} NT=3 batch=512", "Launches", 0, 1, 0, 1, 512),
        # fp64 extra-row split: fits x NT >= 480 inside the mid-size range; not under profiling, not without extra tiles,
        # not for predict after fit (which has one diagonal-free launch per step)
        R(f"{F64} NT=8 batch=59", "Launches", 1, 0, 0, 1, 59),
        R(f"{F64} NT=8 batch=60", "Launches", 1, 0, 1, 1, 60),
        R(f"{F64} NT=8 batch=60 M=130 ET=2", "Launches", 1, 0, 1, 1, 60),
        R(f"{F64} NT=8 batch=60 prof=1", "Launches", 1, 0, 0, 1, 60),
        R(f"{F64} NT=8 batch=60 ET=0", "Launches", 1, 0, 0, 1, 60),
        R(f"{F64} NT=8 batch=60 in_rows=0", "Launches", 1, 1, 0, 1, 60),
        # fp32 group rule: two groups from 56 fits ...
        R(f"{F32} NT=8 batch=55", "Launches", 1, 0, 0, 1, 55, refine="1,1,0"),
        R(f"{F32} NT=8 batch=56", "Launches", 1, 0, 0, 1, (28, 28), tune=1, refine="1,1,0"),
        # ... as long as half the call stays above the latency range (32 fits at two block steps)
        R(f"{F32} NT=2 batch=64", "Launches", 1, 0, 0, 1, 64, refine="1,1,0"),
        R(f"{F32} NT=2 batch=66", "Launches", 1, 0, 0, 1, (33, 33), tune=1, refine="1,1,0"),
        # cgp_set_streams: 0 asks the tuner (whose answer decides), 1 keeps one group, 2 and 4 give two without asking
        R(f"{F32} NT=8 batch=64", "Launches", 1, 0, 0, 1, (32, 32), tune=1, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 tuned_groups=1", "Launches", 1, 0, 0, 1, 64, tune=1, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 tuned_groups=2", "Launches", 1, 0, 0, 1, (32, 32), tune=1, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 nstreams=1", "Launches", 1, 0, 0, 1, 64, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 nstreams=2", "Launches", 1, 0, 0, 1, (32, 32), refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 nstreams=4", "Launches", 1, 0, 0, 1, (32, 32), refine="1,1,0"),
        R(f"{F32} NT=8 batch=40 nstreams=4", "Launches", 1, 0, 0, 1, 40, refine="1,1,0"),
        # one group under profiling and for predict after fit (no refined fit behind it: no refinement either), tuner not asked
        R(f"{F32} NT=8 batch=64 prof=1", "Launches", 1, 0, 0, 1, 64, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 nstreams=2 prof=1", "Launches", 1, 0, 0, 1, 64, refine="1,1,0"),
        R(f"{F32} NT=8 batch=64 in_rows=0", "Launches", 1, 1, 0, 1, 64),
        # outside the mid-size range cgp_set_streams is taken as told: an uneven batch deals its remainder to the first groups
        R(f"{F32} NT=8 batch=97 nstreams=4", "Launches", 0, 0, 0, 1, (25, 24, 24, 24), refine="1,1,0"),
        R(f"{F64} NT=3 batch=53 nstreams=4", "Launches", 0, 0, 0, 1, (14, 13, 13, 13)),
        R(f"{F64} NT=3 batch=53 nstreams=2", "Launches", 0, 0, 0, 1, (27, 26)),
        R(f"{F64} NT=3 batch=53 nstreams=1", "Launches", 0, 0, 0, 1, 53),
        R(f"{F64} NT=3 batch=3 nstreams=99 {THR} mid_cap=0", "Launches", 0, 0, 0, 1, (1, 1, 1)),
        R(f"{F64} NT=3 batch=53 nstreams=4 prof=1", "Launches", 0, 0, 0, 1, 53),
        # an fp64 mid-size call is one group whatever cgp_set_streams says
        R(f"{F64} NT=3 batch=40 nstreams=4", "Launches", 1, 0, 0, 1, 40),
        # use_acc: off for latency (above), without test points, in gradient mode, at one block step (49 fits at NT = 1 above)
        R(f"{F64} NT=3 batch=29 M=0", "Launches", 1, 0, 0, 0, 29),
        R(f"{F64} NT=3 batch=29 xid=1", "Launches", 1, 0, 0, 0, 29),
        # latency capacities: 10 fits x (3 + 1 + 1) slots = 50 units; images from three block steps on
        R(f"{F64} NT=3 batch=10 lat_units=50", "Latency", 1, 0, 0, 0, 10),
        R(f"{F64} NT=3 batch=10 lat_units=49", "Launches", 1, 0, 0, 1, 10),
        R(f"{F64} NT=3 batch=10 lat_img_fits=10", "Latency", 1, 0, 0, 0, 10),
        R(f"{F64} NT=3 batch=10 lat_img_fits=9", "Launches", 1, 0, 0, 1, 10),
        R(f"{F64} NT=2 batch=10 lat_img_fits=1", "Latency", 1, 0, 0, 0, 10),
        R(f"{F64} NT=3 batch=10 lat_cap=9", "Launches", 1, 0, 0, 1, 10),
        R(f"{F64} NT=3 batch=10 lat_images_fit=0", "Launches", 1, 0, 0, 1, 10),
        R(f"{F64} NT=3 batch=10 lat_units=49 mid_cap=9", "Launches", 0, 0, 0, 1, 10),
        R(f"{F64} NT=3 batch=30 mid_cap=29", "Launches", 0, 0, 0, 1, 30),
        # refinement (fp32): a fit call solves for alpha_0 and takes the steps; k_alpha only without refinement
        R(f"{F32} NT=3 batch=2", "Latency", 1, 0, 0, 0, 2, refine="1,1,0"),
        R(f"{F32} NT=3 batch=2 want_alpha=1", "Latency", 1, 0, 0, 0, 2, refine="1,1,1"),
        R(f"{F32} NT=3 batch=2 refine=0", "Latency", 1, 0, 0, 0, 2),
        R(f"{F32} NT=3 batch=2 refine=0 want_alpha=1", "Latency", 1, 0, 0, 0, 2, alpha=1),
        R(f"{F32} NT=3 batch=2 refine=2", "Latency", 1, 0, 0, 0, 2, refine="2,1,0"),
        R(f"{F32} NT=3 batch=2 refine=5", "Latency", 1, 0, 0, 0, 2, refine="3,1,0"),
        R(f"{F32} NT=8 batch=2", "Latency", 1, 0, 0, 0, 2, refine="1,1,0"),
        R(f"{F32} NT=9 batch=2", "Latency", 1, 0, 0, 0, 2, refine="2,1,0"),
        R(f"{F32} NT=3 batch=2 xid=1", "Latency", 1, 0, 0, 0, 2),
        R(f"{F32} NT=3 batch=2 refine_bufs=0", "Latency", 1, 0, 0, 0, 2),
        R(f"{F32} NT=3 batch=2 refine_max_nt=2", "Latency", 1, 0, 0, 0, 2),
        R(f"{F64} NT=3 batch=2 refine_bufs=1 refine_max_nt=100 want_alpha=1", "Latency", 1, 0, 0, 0, 2, alpha=1),
        # predict after fit: the steps on the alpha a refined fit left, nothing after an unrefined one; with alpha asked for, a solve
        R(f"{F32} NT=3 batch=1 in_rows=0 refined=1", "Latency", 1, 1, 0, 0, 1, refine="1,0,0"),
        R(f"{F32} NT=3 batch=1 in_rows=0 refined=0", "Latency", 1, 1, 0, 0, 1),
        R(f"{F32} NT=3 batch=1 in_rows=0 refined=0 want_alpha=1", "Latency", 1, 1, 0, 0, 1, refine="1,1,1"),
        R(f"{F64} NT=3 batch=1 in_rows=0", "Latency", 1, 1, 0, 0, 1),
        # CGP_SCHED=throughput (every build honours it): a handful of fits through the mid-size launches
        R(f"{F64} NT=3 batch=2 {THR}", "Launches", 1, 0, 0, 1, 2),
        R(f"{F32} NT=3 batch=2 {THR}", "Launches", 1, 0, 0, 1, 2, refine="1,1,0"),
        R(f"{F64} NT=1 batch=2 {THR}", "Launches", 1, 0, 0, 0, 2),
    ]
)

# the shipped library knows neither the measurement schedules nor the integer overrides
SHIPPED = [
    R(f"{F64} NT=3 batch=2 {OVERLAP}", "Launches", 1, 0, 0, 1, 2),
    R(f"{F64} NT=3 batch=1 lat_fits_env=0", "Latency", 1, 0, 0, 0, 1),
    R(f"{F64} NT=3 batch=1 mid_fits_env=0", "Latency", 1, 0, 0, 0, 1),
    R(f"{F32} NT=3 batch=40 nstreams=1 xsplit32_env=40", "Launches", 1, 0, 0, 1, 40, refine="1,1,0"),
    R(f"{F32} NT=8 batch=64 nstreams=2 group0_env=20", "Launches", 1, 0, 0, 1, (32, 32), refine="1,1,0"),
]

# the measurement library (-DCGP_AB): the switches of CGP_SCHED / CGP_DIAG / CGP_ACC / CGP_SK_TRMM and the integer overrides
AB = [
    R(f"{F64} NT=3 batch=2 {SPLITDIAG}", "Launches", 1, 1, 0, 1, 2),
    R(f"{F64} NT=8 batch=60 {SPLITDIAG}", "Launches", 1, 1, 0, 1, 60),
    R(f"{F32} NT=3 batch=2 {SPLITDIAG}", "Launches", 1, 1, 0, 1, 2, refine="1,1,0"),
    R(f"{F64} NT=3 batch=512 {FUSEDDIAG}", "Launches", 0, 0, 0, 1, 512),
    R(f"{F64} NT=3 batch=2 {FUSEDDIAG}", "Launches", 1, 0, 0, 1, 2),
    # the two-stream look-ahead: fit calls of one group and two block steps or more, not under profiling
    R(f"{F64} NT=3 batch=2 {OVERLAP}", "LookAhead", 1, 0, 0, 1, 2),
    R(f"{F32} NT=3 batch=2 {OVERLAP}", "LookAhead", 1, 0, 0, 1, 2, refine="1,1,0"),
    R(f"{F64} NT=2 batch=2 {OVERLAP}", "LookAhead", 1, 0, 0, 1, 2),
    R(f"{F64} NT=1 batch=2 {OVERLAP}", "Launches", 1, 0, 0, 0, 2),
    R(f"{F64} NT=3 batch=2 {OVERLAP} prof=1", "Launches", 1, 0, 0, 1, 2),
    R(f"{F64} NT=3 batch=2 {OVERLAP} in_rows=0", "Launches", 1, 1, 0, 1, 2),
    R(f"{F64} NT=3 batch=53 nstreams=2 {OVERLAP}", "Launches", 0, 0, 0, 1, (27, 26)),
    R(f"{F64} NT=3 batch=53 nstreams=1 {OVERLAP}", "LookAhead", 0, 0, 0, 1, 53),
    # the one-launch schedule: mid-size fit calls above the latency range, two block steps or more, SE kernels, not under profiling
    R(f"{F32} NT=5 batch=40 {ONE}", "OneLaunch", 1, 0, 0, 1, 40, refine="1,1,0"),
    R(f"{F64} NT=6 batch=24 {ONE}", "OneLaunch", 1, 0, 0, 1, 24),
    R(f"{F32} NT=8 batch=64 {ONE}", "OneLaunch", 1, 0, 0, 1, (32, 32), tune=1, refine="1,1,0"),
    R(f"{F64} NT=6 batch=22 {ONE}", "Latency", 1, 0, 0, 0, 22),
    R(f"{F64} NT=6 batch=65 {ONE}", "Launches", 0, 0, 0, 1, 65),
    R(f"{F32} NT=1 batch=40 {ONE}", "Launches", 1, 0, 0, 0, 40, refine="1,1,0"),
    R(f"{F64} NT=6 batch=24 {ONE} prof=1", "Launches", 1, 0, 0, 1, 24),
    R(f"{F64} NT=6 batch=24 {ONE} in_rows=0", "Launches", 1, 1, 0, 1, 24),
    R(f"{F64} NT=6 batch=24 {ONE} matern=1", "Launches", 1, 0, 0, 1, 24),
    R(f"{F64} NT=6 batch=24 {ONE} {SPLITDIAG}", "Launches", 1, 1, 0, 1, 24),
    R(f"{F64} NT=6 batch=24 {ONE} {OVERLAP}", "LookAhead", 1, 0, 0, 1, 24),
    R(f"{F64} NT=8 batch=60 {ONE}", "OneLaunch", 1, 0, 1, 1, 60),
    # CGP_ACC=off, CGP_SK_TRMM=fused, CGP_DIAG=fat (no field of the row: it picks a kernel, not a schedule)
    R(f"{F64} NT=3 batch=2 {THR} acc_off=1", "Launches", 1, 0, 0, 0, 2),
    R(f"{F64} NT=3 batch=2 sk_fused_trmm=1", "Latency", 1, 0, 0, 0, 2, trmm=0),
    R(f"{F64} NT=3 batch=2 fat_diag=1", "Latency", 1, 0, 0, 0, 2),
    # CGP_LAT_FITS / CGP_MID_FITS move the crossovers, clamped to what the slabs are sized for (64 / 512 in this library)
    R(f"{F64} NT=3 batch=1 lat_fits_env=0", "Launches", 1, 0, 0, 1, 1),
    R(f"{F64} NT=3 batch=1 lat_fits_env=-5", "Launches", 1, 0, 0, 1, 1),
    R(f"{F64} NT=1 batch=64 lat_fits_env=100 lat_cap=100", "Latency", 0, 0, 0, 0, 64),
    R(f"{F64} NT=1 batch=65 lat_fits_env=100 lat_cap=100", "Launches", 0, 0, 0, 0, 65),
    R(f"{F64} NT=3 batch=29 mid_fits_env=0", "Launches", 0, 0, 0, 1, 29),
    R(f"{F64} NT=3 batch=512 mid_fits_env=9999 mid_cap=600", "Launches", 1, 1, 0, 1, 512),
    R(f"{F64} NT=3 batch=513 mid_fits_env=9999 mid_cap=600", "Launches", 0, 1, 0, 1, 513),
    # CGP_XSPLIT32: fp32 extra rows on the second stream from that many fits, one-group calls only
    R(f"{F32} NT=3 batch=40 nstreams=1 xsplit32_env=40", "Launches", 1, 0, 1, 1, 40, refine="1,1,0"),
    R(f"{F32} NT=3 batch=39 nstreams=1 xsplit32_env=40", "Launches", 1, 0, 0, 1, 39, refine="1,1,0"),
    R(f"{F32} NT=3 batch=40 nstreams=1 xsplit32_env=0", "Launches", 1, 0, 0, 1, 40, refine="1,1,0"),
    R(f"{F32} NT=8 batch=64 xsplit32_env=40", "Launches", 1, 0, 0, 1, (32, 32), tune=1, refine="1,1,0"),
    # CGP_GROUP0: uneven halves of a two-group call
    R(f"{F32} NT=8 batch=64 nstreams=2 group0_env=20", "Launches", 1, 0, 0, 1, (20, 44), refine="1,1,0"),
    R(f"{F32} NT=8 batch=64 nstreams=2 group0_env=64", "Launches", 1, 0, 0, 1, (32, 32), refine="1,1,0"),
]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the table program"
    out = tmp_path_factory.mktemp("sched_plan")
    exe = {}
    for name, flags in (("shipped", []), ("ab", ["-DCGP_AB"])):
        exe[name] = str(out / f"sched_plan_table_{name}")
        subprocess.check_call([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", *flags, "-I", CSRC,
                               os.path.join(ROOT, "tests", "sched_plan_table.cpp"), "-o", exe[name]])
    return exe


def check(exe, rows):
    got = subprocess.run([exe], input="\n".join(w for w, _ in rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(rows)
    wrong = [f"{w}\n   expected {e}\n   got      {g}" for (w, e), g in zip(rows, got) if e != g]
    assert not wrong, "\n".join(wrong)


def test_shipped_library_schedule_table(tables):
    check(tables["shipped"], COMMON + SHIPPED)


def test_measurement_library_schedule_table(tables):
    check(tables["ab"], COMMON + AB)
