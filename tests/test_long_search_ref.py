"""What the long-search inputs (tests/long_search_cases.py) must be, on the oracle alone: the GPU tests of test_long_search_gpu.py
compare bit for bit and would pass just as well on inputs whose searches had all become short.  The bounds are conditions on the
inputs — the figures measured when the cases were designed, with margin — not tolerances on any output."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_ref as R
import long_search_cases as Ls

SHAPES = {"S1": Ls.S1, "S2": Ls.S2}
MIN_SECOND_PASS = {"S1": 0.05, "S2": 0.25}          # share of GOOD matches at least 64 steps into the search


def _trace(oracle, case, imin=None, imax=None):
    col, wgt, gH, eth = Ls.oracle_init(oracle, case["left"], case["u"], case["v"])
    P, d = abi.make_trace_points(len(case["u"]), case["u"], case["v"], col, wgt, gH, eth, imin, imax)
    return Ls.oracle_trace(oracle, case, case["right"], P, 1), d


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_fresh_stereo_matches_lie_in_the_second_pass(oracle, shape):
    case = Ls.stereo_case(SHAPES[shape])
    steps, _ = Ls.stereo_step_count(case)
    assert (steps == (71 if shape == "S1" else 99)).all()
    st, d = _trace(oracle, case)
    good = st == Ls.GOOD
    disp = case["u"][good] - d["lastTraceUV"][good, 0]
    print(shape, "status", np.bincount(st, minlength=6), "share of GOOD with disparity >= 64: %.3f, farthest %.1f" % ((disp >= 64).mean(), disp.max()))
    assert good.sum() > 2000 and (disp >= 64).mean() >= MIN_SECOND_PASS[shape]


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_finite_intervals_take_every_step_count(oracle, shape):
    case = Ls.stereo_case(SHAPES[shape])
    st, d = _trace(oracle, case, case["idepth_min"], case["idepth_max"])
    steps, uMin = Ls.stereo_step_count(case, case["idepth_min"], case["idepth_max"])
    searched = (st == Ls.GOOD) | (st == Ls.OUTLIER)
    hist = np.bincount(steps[searched], minlength=100)
    print(shape, "status", np.bincount(st, minlength=6), "searched points per step count 58..99", hist[58:100])
    if shape == "S1":
        assert (hist[60:71] >= 30).all() and hist[72:].sum() == 0
    else:
        assert (hist[60:99] >= 15).all() and hist[99] >= 300
    good = st == Ls.GOOD
    best = np.abs(d["lastTraceUV"][good, 0] - uMin[good])
    print(shape, "share of GOOD with best step >= 64: %.3f" % (best >= 64.5).mean())
    assert (best >= 64.5).mean() >= (0.01 if shape == "S1" else 0.05)


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_trace_on_matches_lie_in_the_second_pass(oracle, shape):
    case = Ls.trace_on_case(SHAPES[shape])
    n = len(case["u"])
    col, wgt, gH, eth = Ls.oracle_init(oracle, case["host"], case["u"], case["v"])
    P, d = abi.make_trace_points(n, case["u"], case["v"], col, wgt, gH, eth)
    st = np.zeros(n, np.uint8)
    assert oracle.orc_trace_on_batch(abi.fp(case["new"]), case["w"], case["h"], 1, C.byref(case["G"]), abi.ip(np.zeros(n, np.int32)), C.byref(P), abi.bp(st)) == 0
    u0, v0 = Ls.project0(case["KRKi"], case["u"], case["v"])
    good = st == Ls.GOOD
    far = np.hypot(d["lastTraceUV"][good, 0] - u0[good], d["lastTraceUV"][good, 1] - v0[good])
    print(shape, "status", np.bincount(st, minlength=6), "share of GOOD at >= 64.5 px: %.3f, farthest %.1f" % ((far >= 64.5).mean(), far.max()))
    assert good.sum() > 2000 and (far >= 64.5).mean() >= MIN_SECOND_PASS[shape]


@pytest.mark.parametrize("period", [64, 32])
def test_periodic_pair_ties_equal_steps(oracle, period):
    case = Ls.periodic_case(period)
    st, d = _trace(oracle, case)
    good = st == Ls.GOOD
    disp = case["u"][good] - d["lastTraceUV"][good, 0]
    ties = int((d["quality"][good] == 1.0).sum())
    print("period", period, "status", np.bincount(st, minlength=6), "GOOD with quality == 1:", ties, "largest disparity %.2f" % disp.max())
    assert good.sum() >= 300 and ties >= 250
    assert (disp < Ls.MAX_PERIODIC_DISPARITY[period]).all()               # the earliest of the equal steps, every time


@pytest.mark.parametrize("period", [64, 32])
def test_periodic_pair_ties_equal_steps_of_trace_on(oracle, period):
    """the same pair through traceOn (its own step loops, merge and index rule), as a batch and as the resident set's key form"""
    case = Ls.periodic_trace_on_case(period)
    n = len(case["u"])
    P, d = abi.make_trace_points(n, case["u"], case["v"], *Ls.oracle_init(oracle, case["host"], case["u"], case["v"]))
    st = np.zeros(n, np.uint8)
    assert oracle.orc_trace_on_batch(abi.fp(case["new"]), case["w"], case["h"], 1, case["geoms"], abi.ip(np.zeros(n, np.int32)), C.byref(P), abi.bp(st)) == 0
    ref = R.add_frame(oracle, case["host"], case["map"])
    assert len(ref["u"]) == Ls.PERIODIC_RESIDENT_POINTS and len(ref["u"]) % 4 != 0
    R.trace(oracle, [(ref, case["geom"])], case["new"], None, case["K4"], case["Ki"], case["baseline"])
    for name, u, status, uv, quality in (("batch", case["u"], st, d["lastTraceUV"], d["quality"]),
                                         ("resident", ref["u"], ref["lastTraceStatus"], ref["lastTraceUV"], ref["quality"])):
        good = status == Ls.GOOD
        disp = u[good] - uv[good, 0]
        ties = int((quality[good] == 1.0).sum())
        print("period", period, name, "status", np.bincount(status, minlength=6), "GOOD with quality == 1:", ties, "largest disparity %.2f" % disp.max())
        assert good.sum() >= 300 and ties >= 250
        assert (disp < Ls.MAX_PERIODIC_DISPARITY[period]).all()
