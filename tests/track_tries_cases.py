"""Shared by the sdso_track_tries_replay / sdso_track_new_coarse tests: seeded random try lists (event traces), their marshalling into
sdso_track_try_t, the call of the ctx-free replay, and the field-by-field comparison with tests/track_tries_ref.py."""
import ctypes as C

import numpy as np

from sdso_amd import abi
import track_tries_ref as ref

# residuals from a small set, so that equalities (a residual ON a bound, achievedRes[0] ON the stop threshold) and crossings of 1.5 x
# a bound happen all the time; 1e39 is finite as a double and inf as a float (the cast of FullSystem.cpp:476)
RES = [4.0, 4.5, 5.0, 6.0, 6.5, 7.5, 9.0, 11.0, 13.0, 13.5, 20.0]
ODD = [float("inf"), float("nan"), 1e39]
RMSE = [0.0, 3.0, 4.0, 4.0000001, 5.0, 9.0, 1e9, float("nan")]


def random_list(rs):
    """-> (recs, tries, aff_last_2_l, lastCoarseRMSE[5], reTrackThreshold) in the Python form of track_tries_ref"""
    ntries = int(rs.choice([1, 2, 3, 4, 5, 8, 27, 64], p=[0.1, 0.2, 0.2, 0.2, 0.15, 0.1, 0.03, 0.02]))
    top = int(rs.randint(1, 5))                                  # coarsestLvl: every try of a list starts there
    p_good = rs.choice([0.0, 0.3, 0.8, 1.0], p=[0.1, 0.1, 0.6, 0.2])
    recs, tries = [], []
    for k in range(ntries):
        lvls = list(range(top, -1, -1))
        if rs.rand() < 0.5:                                      # one repeated level (haveRepeated: at most one per call)
            j = int(rs.randint(0, len(lvls)))
            lvls.insert(j, lvls[j])
        if rs.rand() < 0.1:                                      # the try ended early when it ran (an abort under the bounds it ran with)
            lvls = lvls[:int(rs.randint(0, len(lvls) + 1))]
            good = 0
        else:
            good = int(rs.rand() < p_good)
        ev = []
        for l in lvls:
            r = float(rs.choice(ODD)) if rs.rand() < 0.06 else float(rs.choice(RES))
            ev.append((l, r, tuple(float(x) for x in rs.normal(0, 3, 3))))
        recs.append(dict(events=ev, end_good=good, end_pose=tuple(rs.normal(0, 1, 12)), end_aff=tuple(rs.normal(0, 1, 2))))
        tries.append(tuple(rs.normal(0, 1, 12)))
    rmse = [float(rs.choice(RMSE))] + [float(x) for x in rs.normal(5, 1, 4)]
    return recs, tries, tuple(rs.normal(0, 1, 2)), rmse, float(rs.choice([1.5, 1.0, 2.0], p=[0.8, 0.1, 0.1]))


def se3_of(v):
    s = abi.SE3()
    s.R[:] = list(v[:9]); s.t[:] = list(v[9:])
    return s


def se3_tuple(s):
    return tuple(s.R[:]) + tuple(s.t[:])


def to_c(recs, tries):
    n = len(recs)
    R = (abi.TrackTry * n)()
    T = (abi.SE3 * n)(*[se3_of(t) for t in tries])
    for k, r in enumerate(recs):
        R[k].trace.n = len(r["events"])
        for e, (lvl, res, flow) in enumerate(r["events"]):
            R[k].trace.lvl[e] = lvl; R[k].trace.res[e] = res
            R[k].trace.flow[e][:] = list(flow)
        R[k].end_good = r["end_good"]; R[k].end_pose = se3_of(r["end_pose"]); R[k].end_aff = abi.Aff(*r["end_aff"])
    return R, T


def from_c(R):
    """the `in` members of returned records, in the Python form"""
    return [dict(events=[(r.trace.lvl[e], r.trace.res[e], tuple(r.trace.flow[e][:])) for e in range(r.trace.n)], end_good=r.end_good,
                 end_pose=se3_tuple(r.end_pose), end_aff=(r.end_aff.a, r.end_aff.b)) for r in R]


def replay(L, R, T, aff0, rmse, thr):
    """sdso_track_tries_replay -> (rc, result, lastCoarseRMSE out)"""
    out = abi.TrackTriesResult()
    rm = (C.c_double * 5)(*rmse)
    a = abi.Aff(*aff0)
    rc = L.sdso_track_tries_replay(len(R), T, C.byref(a), R, rm, thr, C.byref(out))
    return rc, out, list(rm)


def assert_equal_to_ref(out, rm, R, want, what=""):
    """every output of the C side against track_tries_ref.track_new_coarse: integers exactly, doubles bit for bit"""
    same = ref.same_double
    assert (out.haveOneGood, out.winner, out.tryIterations) == (want["haveOneGood"], want["winner"], want["tryIterations"]), what
    assert all(same(a, b) for a, b in zip(se3_tuple(out.pose), want["pose"])), what
    assert same(out.aff.a, want["aff"][0]) and same(out.aff.b, want["aff"][1]), what
    assert all(same(a, b) for a, b in zip(out.flowVecs[:], want["flowVecs"])), what
    assert all(same(a, b) for a, b in zip(out.achievedRes[:], want["achievedRes"])), what
    assert all(same(a, b) for a, b in zip(rm, want["lastCoarseRMSE"])), what
    for k, s in enumerate(want["seen"]):
        if s is None:
            assert R[k].ran == 0, (what, k)
            continue
        r = R[k]
        assert (r.ran, r.good, r.abort_lvl, r.winner) == (1, s["good"], s["abort_lvl"], s["winner"]), (what, k)
        assert all(same(a, b) for a, b in zip(r.lastResiduals[:], s["lastResiduals"])), (what, k)
        assert all(same(a, b) for a, b in zip(r.lastFlowIndicators[:], s["lastFlowIndicators"])), (what, k)
        assert all(same(a, b) for a, b in zip(se3_tuple(r.pose), s["pose"])), (what, k)
        assert same(r.aff.a, s["aff"][0]) and same(r.aff.b, s["aff"][1]), (what, k)


# ---- the GPU tests' problem and starts (tests/test_track_tries_gpu.py, tests/test_track_tries_shim_gpu.py)
TRUTH = np.array([0.02, -0.01, 0.35, 0.004, -0.006, 0.002])      # Sophus tangent of the small problem's motion
G = TRUTH + np.array([0.01, -0.01, 0.05, 0.002, 0.001, -0.002])  # a start that converges
H = np.array([3.0, 0, 0, 0, 0.5, 0])                             # the hopeless start of test_track_hypotheses_in_lock_step
REF_SLOT, NEW_SLOT = 1, 2


def problem():
    import synth
    return synth.tracker_problem(w=640, h=480, npts=2000, seed=2001)


def poses(tangents):
    """tangents -> 12-tuples (R row-major, t), the form of `tries` everywhere in this module"""
    import synth
    out = []
    for xi in tangents:
        R, t = synth.se3_exp(np.asarray(xi, np.float64))
        out.append(tuple(np.asarray(R, np.float64).reshape(9)) + tuple(np.asarray(t, np.float64)))
    return out


def new_coarse(ctx, prm, tries, aff0, rmse, thr=1.5, ref_slot=REF_SLOT, new_slot=NEW_SLOT, with_recs=True):
    """sdso_track_new_coarse -> (rc, result, lastCoarseRMSE out, records or None)"""
    n = len(tries)
    T = (abi.SE3 * n)(*[se3_of(t) for t in tries])
    R = (abi.TrackTry * n)() if with_recs else None
    out = abi.TrackTriesResult()
    rm = (C.c_double * 5)(*rmse)
    a = abi.Aff(*aff0)
    rc = ctx.L.sdso_track_new_coarse(ctx.h, ref_slot, new_slot, C.byref(prm), n, T, C.byref(a), rm, thr, C.byref(out), R)
    return rc, out, list(rm), R


class OracleTracker:
    """the oracle's trackNewestCoarse behind track_tries_ref.MockTracker's interface"""

    def __init__(self, orc, prob, prm):
        import helpers
        self.orc, self.prob, self.helpers = orc, prob, helpers
        self.prm = abi.TrackParams.from_buffer_copy(bytes(prm))
        self.lastResiduals = [float("nan")] * 5
        self.lastFlowIndicators = [1000.0] * 3

    def trackNewestCoarse(self, _rec, lastToNew, aff_g2l, minResForAbort):
        for i in range(5):
            self.prm.minResForAbort[i] = minResForAbort[i]
        T0 = (np.array(lastToNew[:9]).reshape(3, 3), np.array(lastToNew[9:]))
        T, aff, out = self.helpers.oracle_track(self.orc, self.prob, self.prm, T0, aff_g2l)
        self.lastResiduals = list(out.lastResiduals)
        self.lastFlowIndicators = list(out.lastFlowIndicators)
        # the level an abort fired on: the finest level reached, where the call ended not good with its references untouched
        reached = [l for l in range(5) if not np.isnan(out.lastResiduals[l])]
        aborted = (not out.good) and reached and min(reached) > 0
        return bool(out.good), se3_tuple(T), (aff.a, aff.b), (min(reached) if aborted else -1)


def oracle_loop(orc, prob, prm, tries, aff0, rmse, thr=1.5):
    """FullSystem.cpp:436-511 over the oracle's trackNewestCoarse (the Python loop of track_tries_ref)"""
    return ref.track_new_coarse([None] * len(tries), tries, aff0, rmse, thr, tracker=OracleTracker(orc, prob, prm))
