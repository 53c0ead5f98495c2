"""Shared by the sdso_g2o_track_newest_coarse_batch / sdso_g2o_track_new_coarse tests: the fork-live variant of
track_tries_cases.OracleTracker (the same class calling orc_g2o_track_newest_coarse), the calls through ctypes, and the project's bars for
the fork-live tracker (tests/test_g2o_factors.py::test_gpu_g2o_tracker_matches_oracle)."""
import ctypes as C

import numpy as np

from sdso_amd import abi
import track_tries_cases as cases
import track_tries_ref as ref

ORC_FN = "orc_g2o_track_newest_coarse"
POSE_TOL, A_TOL, B_TOL, RES_RTOL = 1e-9, 1e-9, 1e-7, 1e-6


class OracleTracker(cases.OracleTracker):
    """the oracle's fork-live trackNewestCoarse behind track_tries_ref.MockTracker's interface"""

    def trackNewestCoarse(self, _rec, lastToNew, aff_g2l, minResForAbort):
        for i in range(5):
            self.prm.minResForAbort[i] = minResForAbort[i]
        T0 = (np.array(lastToNew[:9]).reshape(3, 3), np.array(lastToNew[9:]))
        T, aff, out = self.helpers.oracle_track(self.orc, self.prob, self.prm, T0, aff_g2l, fn=ORC_FN)
        self.lastResiduals = list(out.lastResiduals)
        self.lastFlowIndicators = list(out.lastFlowIndicators)
        reached = [l for l in range(5) if not np.isnan(out.lastResiduals[l])]
        aborted = (not out.good) and reached and min(reached) > 0
        return bool(out.good), cases.se3_tuple(T), (aff.a, aff.b), (min(reached) if aborted else -1)


def oracle_loop(orc, prob, prm, tries, aff0, rmse, thr=1.5):
    """FullSystem.cpp:436-511 over the oracle's fork-live trackNewestCoarse (the Python loop of track_tries_ref)"""
    return ref.track_new_coarse([None] * len(tries), tries, aff0, rmse, thr, tracker=OracleTracker(orc, prob, prm))


def oracle_single(orc, prob, prm, pose, aff0):
    """one oracle call from a 12-tuple pose -> (pose 12-tuple, (a, b), TrackResult)"""
    import helpers
    T0 = (np.array(pose[:9]).reshape(3, 3), np.array(pose[9:]))
    T, aff, out = helpers.oracle_track(orc, prob, prm, T0, aff0, fn=ORC_FN)
    return cases.se3_tuple(T), (aff.a, aff.b), out


def host_single(ctx, prm, pose, aff0, ref_slot=cases.REF_SLOT, new_slot=cases.NEW_SLOT):
    """sdso_g2o_track_newest_coarse, the host-driven call -> (rc, pose 12-tuple, (a, b), TrackResult)"""
    T = cases.se3_of(pose); aff = abi.Aff(*aff0); out = abi.TrackResult()
    rc = ctx.L.sdso_g2o_track_newest_coarse(ctx.h, ref_slot, new_slot, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out))
    return rc, cases.se3_tuple(T), (aff.a, aff.b), out


def batch(ctx, prms, poses, affs, ref_slot=cases.REF_SLOT, new_slot=cases.NEW_SLOT):
    """sdso_g2o_track_newest_coarse_batch -> (rc, SE3 array, Aff array, TrackResult array)"""
    n = len(poses)
    P = (abi.TrackParams * n)(*[abi.TrackParams.from_buffer_copy(bytes(p)) for p in prms])
    T = (abi.SE3 * n)(*[cases.se3_of(t) for t in poses])
    A = (abi.Aff * n)(*[abi.Aff(*a) for a in affs])
    O = (abi.TrackResult * n)()
    refs = (C.c_int * n)(*([ref_slot] * n)); frames = (C.c_int * n)(*([new_slot] * n))
    rc = ctx.L.sdso_g2o_track_newest_coarse_batch(ctx.h, n, refs, frames, P, T, A, O)
    return rc, T, A, O


def new_coarse(ctx, prm, tries, aff0, rmse, thr=1.5, ref_slot=cases.REF_SLOT, new_slot=cases.NEW_SLOT, with_recs=True):
    """sdso_g2o_track_new_coarse -> (rc, result, lastCoarseRMSE out, records or None)"""
    n = len(tries)
    T = (abi.SE3 * n)(*[cases.se3_of(t) for t in tries])
    R = (abi.TrackTry * n)() if with_recs else None
    out = abi.TrackTriesResult()
    rm = (C.c_double * 5)(*rmse)
    a = abi.Aff(*aff0)
    rc = ctx.L.sdso_g2o_track_new_coarse(ctx.h, ref_slot, new_slot, C.byref(prm), n, T, C.byref(a), rm, thr, C.byref(out), R)
    return rc, out, list(rm), R


def ints_of(out):
    return (out.good, list(out.iterations), out.evaluations, out.point_evals)


def res_close(got, want):
    """residual vectors: the same NaN pattern, finite entries within RES_RTOL relative"""
    g, w = np.array(list(got), np.float64), np.array(list(want), np.float64)
    return bool(np.array_equal(np.isnan(g), np.isnan(w)) and np.allclose(g, w, rtol=RES_RTOL, atol=0, equal_nan=True))


def estimate_close(pose, aff, want_pose, want_aff):
    return bool(np.abs(np.array(pose) - np.array(want_pose)).max() <= POSE_TOL and abs(aff[0] - want_aff[0]) <= A_TOL and abs(aff[1] - want_aff[1]) <= B_TOL)


def in_members(r):
    """the `in` members of a record as bytes: the try as it ran"""
    return bytes(r.trace) + bytes(C.c_int(r.end_good)) + bytes(r.end_pose) + bytes(r.end_aff)
