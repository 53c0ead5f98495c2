"""The CPU statement of the stereo initialiser (tests/init_ref.py): its two rules walked on hand-made trace results, and the conditions the
GPU cases (tests/test_init_gpu.py) rely on, asserted on their inputs with the CPU oracle."""
import numpy as np
import pytest

import immature_ref as R
import init_cases as IC
import init_ref as IR

f32 = np.float32
nan, inf = np.nan, np.inf
ETH = 8 * 144.0
# a 24 x 20 map: the walked area is x in [3, 20), y in [3, 16).  (x, y, type, status, energyTH, idepth_min, idepth_max, idepth_stereo)
HAND = (
    (3, 3, 1, R.GOOD, ETH, 0.1, 0.2, 0.15),                # the first walked pixel: a Pnt at idepth_stereo, a point
    (19, 3, 2, R.GOOD, ETH, -0.05, 0.1, 0.02),             # GOOD with idepth_min_stereo < 0: a Pnt at idepth_stereo, dropped in STEP 3
    (10, 7, 4, R.OOB, ETH, 0.0, nan, 0.0),                 # 0.01, dropped (idepth_max NaN)
    (11, 7, 1, R.OUTLIER, ETH, -0.3, -0.1, 0.0),           # OUTLIER with a finite interval and idepth_max_stereo < 0 (ImmaturePoint.cpp:440-443)
    (12, 7, 2, R.OUTLIER, ETH, 0.0, nan, 0.0),             # OUTLIER by its energy: the interval was never written
    (4, 9, 4, R.OUTLIER, nan, 0.0, nan, 0.0),              # a non-finite energyTH still becomes a Pnt
    (5, 9, 1, R.SKIPPED, ETH, 0.0, nan, 0.0),
    (6, 9, 2, R.BADCONDITION, ETH, 0.0, nan, 0.0),
    (7, 15, 4, R.GOOD, ETH, 0.0, 0.3, 0.25),               # the last walked row; idepth_min == 0 is not < 0: a point
    (8, 15, 1, R.GOOD, inf, 0.1, 0.2, 0.15),               # each term of :1552-1555 alone
    (9, 15, 2, R.GOOD, ETH, 0.1, inf, 0.15),
    (10, 15, 4, R.GOOD, ETH, -inf, 0.2, 0.15),
    (19, 15, 1, R.GOOD, ETH, 0.2, 0.4, 0.3),               # the last walked pixel
)
EXCLUDED = ((1, 1), (2, 3), (3, 2), (20, 5), (5, 16), (23, 19))   # selected, but outside the walked area


def _hand_map():
    m = np.zeros((20, 24), f32)
    for x, y, t, *_ in HAND:
        m[y, x] = t
    for x, y in EXCLUDED:
        m[y, x] = 2
    return m


def _hand_trace(u, v):
    by_px = {(x, y): r for x, y, *r in HAND}
    rows = [by_px[(int(a), int(b))] for a, b in zip(u, v)]
    col = lambda k, dt=f32: np.array([r[k] for r in rows], dt)
    n = len(rows)
    return dict(status=col(1, np.uint8), energyTH=col(2), idepth_min=col(3), idepth_max=col(4), idepth_stereo=col(5),
                color=np.arange(n * 8, dtype=f32).reshape(n, 8), weights=-np.arange(n * 8, dtype=f32).reshape(n, 8))


def test_the_pnt_rule_on_hand_made_traces():
    S = IR.set_first_with(_hand_map(), _hand_trace)
    order = sorted(range(len(HAND)), key=lambda k: (HAND[k][1], HAND[k][0]))         # raster order
    assert order == list(range(len(HAND)))
    P = S["pnts"]
    assert S["n"] == len(HAND) and list(P["u"]) == [r[0] for r in HAND] and list(P["v"]) == [r[1] for r in HAND]
    assert list(P["my_type"]) == [r[2] for r in HAND] and list(P["status"]) == [r[3] for r in HAND]
    want = [f32(r[7]) if r[3] == R.GOOD else f32(0.01) for r in HAND]
    assert list(P["idepth"]) == want and list(P["iR"]) == want
    assert np.isnan(S["kept"]["energyTH"][5]) and P["idepth"][5] == f32(0.01)       # not dropped here
    assert list(S["counts"]) == [len(HAND) + len(EXCLUDED), len(HAND), 7, 1, 3, 1, 1, 0]


def test_step_3_on_hand_made_traces():
    S = IR.set_first_with(_hand_map(), _hand_trace)
    F = IR.from_initializer(S)
    assert list(F["points"]["pnt"]) == [0, 8, 12] and list(F["counts"]) == [13, 0, 10, 3]
    assert list(F["points"]["idepth"]) == [f32(0.15), f32(0.25), f32(0.3)] and list(F["points"]["idepth_min"]) == [f32(0.1), f32(0), f32(0.2)]
    assert list(F["points"]["u"]) == [3, 7, 19] and list(F["points"]["my_type"]) == [1, 4, 1]
    assert np.array_equal(F["points"]["color"], S["kept"]["color"][[0, 8, 12]]) and np.array_equal(F["points"]["weights"], S["kept"]["weights"][[0, 8, 12]])
    keep = np.ones(13, np.uint8)
    keep[[0, 1, 5]] = 0                        # a point-to-be and two Pnts the filter would drop anyway: skipped, not dropped
    G = IR.from_initializer(S, keep)
    assert list(G["points"]["pnt"]) == [8, 12] and list(G["counts"]) == [13, 3, 8, 2]
    assert list(IR.from_initializer(S, np.zeros(13, np.uint8))["counts"]) == [13, 13, 0, 0]
    assert IR.same(IR.from_initializer(S)["points"], F["points"], IR.POINT) is None     # the state is not changed


def test_an_empty_walk():
    m = IC.border_only_map(640, 480)
    S = IR.set_first_with(m, _hand_trace)
    assert S["n"] == 0 and list(S["counts"]) == [len(IC.BORDER(640, 480)), 0, 0, 0, 0, 0, 0, 0]
    assert list(IR.from_initializer(S)["counts"]) == [0, 0, 0, 0]


# ---- the conditions of the GPU cases, on the CPU oracle.  IPS_SKIPPED and IPS_BADCONDITION need a finite idepth_max_stereo on entry
# (ImmaturePoint.cpp:161 sits in the finite branch, :212 tests it), which a fresh point never has: they cannot occur in a setFirstStereo trace and are not forced.
TABLE = {(640, 480): dict(made=9205, pnts=9205, hist=[8794, 246, 165, 0, 0, 0], neg_min=174, outlier_finite=25, survivors=8645),
         (320, 240): dict(made=1946, pnts=1900, hist=[1704, 91, 105, 0, 0, 0], neg_min=102, outlier_finite=15, survivors=1617)}


@pytest.mark.parametrize("size", IC.SIZES)
def test_conditions_of_the_gpu_cases(oracle, size):
    w, h = size
    P = IC.stereo_pair(w, h)
    made, m = IR.select(oracle, P["pyr_left"], IC.density(w, h))
    S = IR.set_first_with(m, IR.trace_first(oracle, P["pyr_left"][0], P["right"], P["K4"], P["baseline"]))
    K, st = S["kept"], S["pnts"]["status"]
    finite = np.isfinite(K["idepth_min"]) & np.isfinite(K["idepth_max"])
    F = IR.from_initializer(S)
    got = dict(made=made, pnts=S["n"], hist=list(S["counts"][2:]), neg_min=int((finite & (K["idepth_min"] < 0)).sum()),
               outlier_finite=int(((st == R.OUTLIER) & finite).sum()), survivors=F["n"])
    print(size, got)
    assert got == TABLE[size]
    assert made == int((m != 0).sum()) and S["n"] % 64 != 0 and S["n"] % 256 != 0
    assert min(got["hist"][:3]) > 0 and got["neg_min"] > 0 and got["outlier_finite"] > 0
    assert got["hist"][R.SKIPPED] == 0 and got["hist"][R.BADCONDITION] == 0 and got["hist"][R.UNINITIALIZED] == 0
    assert ((st == R.GOOD) & (K["idepth_min"] < 0)).any()                                # GOOD, yet dropped in STEP 3
    assert (K["idepth_max"][(st == R.OUTLIER) & finite] < 0).all()                        # ImmaturePoint.cpp:440-443 is the only such exit
    assert (st[F["points"]["pnt"]] == R.GOOD).all() and np.isfinite(F["points"]["idepth"]).all()   # no survivor reads an unset idepth_stereo
    if size == (320, 240):
        assert S["n"] < made and IC.DESIRED_POINT_DENSITY / S["n"] > 1                   # border pixels skipped; keepPercentage > 1 keeps every Pnt
    else:
        keep = IC.keep_flags(S["n"], 5, IC.DESIRED_POINT_DENSITY / S["n"])
        assert 0.15 * S["n"] < keep.sum() < 0.3 * S["n"]


def test_conditions_of_the_crafted_case(oracle):
    c = IC.crafted_case()
    w, h = c["w"], c["h"]
    S = IR.set_first_with(c["map"], IR.trace_first(oracle, c["left"], c["right"], c["K4"], c["baseline"]))
    P = S["pnts"]
    assert S["counts"][0] - S["n"] == len(IC.BORDER(w, h)) and set(np.unique(P["my_type"])) == {1.0, 2.0, 4.0}
    assert P["u"].min() == 3 and P["u"].max() == w - 5 and P["v"].min() == 3 and P["v"].max() == h - 5       # one pixel just inside each side
    bad = np.nonzero(~np.isfinite(S["kept"]["energyTH"]))[0]
    assert len(bad) >= 3 and set(c["bad"]) <= set(bad)
    assert (P["idepth"][bad] == f32(0.01)).all() and (P["status"][bad] != R.GOOD).all()                      # Pnts all the same
    assert not set(bad) & set(IR.from_initializer(S)["points"]["pnt"])                                        # and dropped in STEP 3
