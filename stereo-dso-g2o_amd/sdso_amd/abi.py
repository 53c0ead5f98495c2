"""ctypes view of include/sdso_abi.h: structure layouts and the loader for libsdso_hip.so.

There is no CPU fallback: load() raises if the HIP library has not been built, and Context()
raises if no MI355X/HIP device is usable.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDSO_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libsdso_hip.so")   # override: A/B experiments only

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_u8_p = C.POINTER(C.c_uint8)


class TrackEval(C.Structure):
    _fields_ = [("lvl", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Ki", C.c_float * 9), ("RKi", C.c_float * 9), ("t", C.c_float * 3),
                ("affLL", C.c_float * 2), ("ref_b0", C.c_float), ("cutoffTH", C.c_float),
                ("huberTH", C.c_float)]


class SE3(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]

    @staticmethod
    def from_Rt(R, t):
        s = SE3()
        s.R[:] = np.asarray(R, np.float64).reshape(9).tolist()
        s.t[:] = np.asarray(t, np.float64).reshape(3).tolist()
        return s

    def Rt(self):
        return np.array(self.R[:]).reshape(3, 3), np.array(self.t[:])


class Aff(C.Structure):
    _fields_ = [("a", C.c_double), ("b", C.c_double)]


class TrackParams(C.Structure):
    _fields_ = [("levels", C.c_int), ("w", C.c_int * 6), ("h", C.c_int * 6),
                ("fx", C.c_float * 6), ("fy", C.c_float * 6), ("cx", C.c_float * 6), ("cy", C.c_float * 6),
                ("ref_exposure", C.c_float), ("new_exposure", C.c_float), ("ref_aff_g2l", Aff),
                ("coarsestLvl", C.c_int), ("minResForAbort", C.c_double * 5),
                ("coarseCutoffTH", C.c_float), ("huberTH", C.c_float), ("maxIterations", C.c_int * 5),
                ("affineOptModeA", C.c_double), ("affineOptModeB", C.c_double)]


class TrackResult(C.Structure):
    _fields_ = [("good", C.c_int), ("lastResiduals", C.c_double * 5), ("lastFlowIndicators", C.c_double * 3),
                ("iterations", C.c_int * 5), ("evaluations", C.c_int), ("point_evals", C.c_longlong)]


class TrackTrace(C.Structure):
    """sdso_track_trace_t: the finish_level events of one try."""
    _fields_ = [("n", C.c_int), ("lvl", C.c_int * 6), ("res", C.c_double * 6), ("flow", (C.c_double * 3) * 6)]


class TrackTry(C.Structure):
    """sdso_track_try_t: one try of FullSystem::trackNewCoarse's loop — as it ran (trace, end_*) and as the loop saw it."""
    _fields_ = [("trace", TrackTrace), ("end_good", C.c_int), ("end_pose", SE3), ("end_aff", Aff),
                ("ran", C.c_int), ("good", C.c_int), ("abort_lvl", C.c_int), ("winner", C.c_int),
                ("lastResiduals", C.c_double * 5), ("lastFlowIndicators", C.c_double * 3), ("pose", SE3), ("aff", Aff)]


class TrackTriesResult(C.Structure):
    """sdso_track_tries_result_t"""
    _fields_ = [("haveOneGood", C.c_int), ("winner", C.c_int), ("tryIterations", C.c_int), ("pose", SE3), ("aff", Aff),
                ("flowVecs", C.c_double * 3), ("achievedRes", C.c_double * 5)]


class BAWindow(C.Structure):
    _fields_ = [("nf", C.c_int), ("np", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("calib_value_scaled", C.c_double * 4), ("calib_value_zero", C.c_double * 4),
                ("evalPT", c_double_p), ("state", c_double_p), ("state_zero", c_double_p),
                ("ab_exposure", c_float_p), ("frameEnergyTH", c_float_p), ("frameID", c_int_p),
                ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("u", c_float_p), ("v", c_float_p), ("idepth", c_float_p), ("idepth_zero", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("host", c_int_p), ("hasDepthPrior", c_u8_p),
                ("res_point", c_int_p), ("res_target", c_int_p), ("res_state", c_u8_p),
                ("HM", c_double_p), ("bM", c_double_p),
                ("solverMode", C.c_int), ("affineOptModeA", C.c_double), ("affineOptModeB", C.c_double),
                ("forceAcceptStep", C.c_int),
                ("maxRelBaseline", c_float_p), ("numGoodResiduals", c_int_p), ("res_isNew", c_u8_p)]


class BAWindowEdit(C.Structure):
    """sdso_ba_window_edit_t: the seven stages of sdso_ba_window_update (include/sdso_abi.h)."""
    _fields_ = [("n_drop_res", C.c_int), ("drop_res", c_int_p),
                ("n_remove_points", C.c_int), ("remove_points", c_int_p),
                ("drop_point", c_u8_p),
                ("n_remove_frames", C.c_int), ("remove_frames", c_int_p),
                ("n_add_frames", C.c_int), ("evalPT", c_double_p), ("state", c_double_p), ("state_zero", c_double_p),
                ("ab_exposure", c_float_p), ("frameEnergyTH", c_float_p), ("frameID", c_int_p), ("frame_slot", c_int_p),
                ("n_add_res", C.c_int), ("add_res_point", c_int_p), ("add_res_target", c_int_p), ("add_res_state", c_u8_p), ("add_res_isNew", c_u8_p),
                ("n_add_points", C.c_int), ("pt_host", c_int_p),
                ("pt_u", c_float_p), ("pt_v", c_float_p), ("pt_idepth", c_float_p), ("pt_idepth_zero", c_float_p),
                ("pt_color", c_float_p), ("pt_weights", c_float_p),
                ("pt_hasDepthPrior", c_u8_p), ("pt_maxRelBaseline", c_float_p), ("pt_numGoodResiduals", c_int_p),
                ("n_pt_res", C.c_int), ("pt_res_point", c_int_p), ("pt_res_target", c_int_p), ("pt_res_state", c_u8_p), ("pt_res_isNew", c_u8_p)]


# sdso_comm_init_host's transport callbacks (include/sdso_abi.h)
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_size_t)
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t)


class BAOptResult(C.Structure):
    _fields_ = [("iterations", C.c_int), ("lastEnergy", C.c_double), ("rmse", C.c_double), ("resInA", C.c_int)]


class BAPostState(C.Structure):
    """sdso_ba_post_state_t: what FullSystem::optimize leaves behind (FullSystemOptimize.cpp:52-87, :142-203, :997-1041)."""
    _fields_ = [("idepth", c_float_p), ("step", c_float_p), ("HdiF", c_float_p), ("bdSumF", c_float_p), ("idepth_hessian", c_float_p),
                ("maxRelBaseline", c_float_p), ("numGoodResiduals", c_int_p),
                ("state_state", c_u8_p), ("isActiveAndIsGoodNEW", c_u8_p), ("state_energy", c_float_p), ("centerProjectedTo", c_float_p),
                ("projectedTo", c_float_p), ("toRemove", c_u8_p),
                ("state", c_double_p), ("state_zero", c_double_p), ("evalPT", c_double_p), ("PRE_worldToCam", c_double_p),
                ("frame_step", c_double_p), ("frameEnergyTH", c_float_p),
                ("calib_value", C.c_double * 4), ("calib_value_scaled", C.c_double * 4), ("calib_step", C.c_double * 4),
                ("lastX", c_double_p), ("lastHS", c_double_p), ("lastbS", c_double_p),
                ("resInA", C.c_int), ("resInL", C.c_int), ("resInM", C.c_int), ("n_toRemove", C.c_int), ("result", BAOptResult)]


def make_post_state(nf, npts, nr, with_system=True):
    """A BAPostState with every array allocated; returns (struct, dict of numpy arrays)."""
    n = 8 * nf + 4
    d = dict(idepth=np.zeros(npts, np.float32), step=np.zeros(npts, np.float32), HdiF=np.zeros(npts, np.float32), bdSumF=np.zeros(npts, np.float32),
             idepth_hessian=np.zeros(npts, np.float32), maxRelBaseline=np.zeros(npts, np.float32), numGoodResiduals=np.zeros(npts, np.int32),
             state_state=np.zeros(nr, np.uint8), isActiveAndIsGoodNEW=np.zeros(nr, np.uint8), state_energy=np.zeros(nr, np.float32),
             centerProjectedTo=np.zeros((nr, 3), np.float32), projectedTo=np.zeros((nr, 16), np.float32), toRemove=np.zeros(nr, np.uint8),
             state=np.zeros((nf, 10)), state_zero=np.zeros((nf, 10)), evalPT=np.zeros((nf, 12)), PRE_worldToCam=np.zeros((nf, 12)),
             frame_step=np.zeros((nf, 10)), frameEnergyTH=np.zeros(nf, np.float32), lastX=np.zeros(n))
    if with_system:
        d["lastHS"] = np.zeros((n, n)); d["lastbS"] = np.zeros(n)
    P = BAPostState()
    for k, a in d.items():
        setattr(P, k, {np.dtype(np.float32): fp, np.dtype(np.float64): dp, np.dtype(np.int32): ip, np.dtype(np.uint8): bp}[a.dtype](a))
    return P, d


PT_KEEP, PT_DROP_NO_RESIDUAL, PT_DROP_NEGATIVE, PT_MARGINALIZE, PT_DROP_WEAK, PT_DROP_NOT_INLIER = range(6)   # SDSO_PT_*


class BAFlagPoints(C.Structure):
    """sdso_ba_flag_points_t: removeOutliers + flagPointsForRemoval on the resident window (FullSystem.cpp:965-1056)."""
    _fields_ = [("frame_marg", c_u8_p), ("last_gone", c_u8_p), ("minGoodActiveResForMarg", C.c_int), ("minGoodResForMarg", C.c_int),
                ("minIdepthH_marg", C.c_float)]


def make_flag_points(frame_marg, last_gone=None, minGoodActiveResForMarg=3, minGoodResForMarg=4, minIdepthH_marg=50.0):
    """Fill a BAFlagPoints.  frame_marg: nf flags; last_gone: np*2 bytes (0/1/2 or 255) or None.  Returns (struct, keep-alive list)."""
    F = BAFlagPoints()
    keep = [np.ascontiguousarray(frame_marg, np.uint8)]
    F.frame_marg = bp(keep[0])
    if last_gone is not None:
        keep.append(np.ascontiguousarray(last_gone, np.uint8).reshape(-1))
        F.last_gone = bp(keep[1])
    F.minGoodActiveResForMarg, F.minGoodResForMarg, F.minIdepthH_marg = int(minGoodActiveResForMarg), int(minGoodResForMarg), float(minIdepthH_marg)
    return F, keep


class MapUpdate(C.Structure):
    """sdso_map_update_t: the orders of a keyframe's point lists (window point indices)."""
    _fields_ = [("n_active", C.c_int), ("active", c_int_p), ("n_gone", C.c_int), ("gone", c_int_p), ("gone_list", c_u8_p)]


class MapCloud(C.Structure):
    """sdso_map_cloud_t: KeyFrameDisplay::refreshPC for up to 8 keyframes."""
    _fields_ = [("n_frames", C.c_int), ("frameID", c_int_p), ("imm_host_id", c_int_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("scaledTH", C.c_float), ("absTH", C.c_float), ("minBS", C.c_float), ("mode", C.c_int), ("camToWorld", c_float_p),
                ("cap", C.c_int)]


MAP_REC_FLOATS = 16          # u, v, idepth, idepth_hessian, maxRelBaseline, color[8], padding (csrc/map_cloud.h)


class TracePoints(C.Structure):
    _fields_ = [("n", C.c_int), ("u_stereo", c_float_p), ("v_stereo", c_float_p), ("idepth_min", c_float_p),
                ("idepth_min_stereo", c_float_p), ("idepth_max_stereo", c_float_p), ("idepth_stereo", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("gradH", c_float_p), ("energyTH", c_float_p),
                ("quality", c_float_p), ("lastTraceStatus", c_u8_p), ("lastTraceUV", c_float_p),
                ("lastTracePixelInterval", c_float_p)]


class TraceGeom(C.Structure):
    _fields_ = [("KRKi", C.c_float * 9), ("Kt", C.c_float * 3), ("aff", C.c_float * 2)]


class ImmGeom(C.Structure):
    """sdso_imm_geom_t: the geometry of one host keyframe into the newest frame (FullSystem.cpp:654-665)."""
    _fields_ = [("host_id", C.c_int), ("KRKi", C.c_float * 9), ("Kt", C.c_float * 3), ("aff", C.c_float * 2), ("KRi", C.c_float * 9), ("t", C.c_float * 3)]


INIT_NCOUNTS = 8   # non-zero map entries, numPoints[0], the histogram of the returned ImmaturePointStatus 0..5 over the Pnts


class InitPnts(C.Structure):
    """sdso_init_pnts_t: the Pnt members of CoarseInitializer::points[0] (CoarseInitializer.cpp:905-969)."""
    _fields_ = [("n", C.c_int), ("u", c_float_p), ("v", c_float_p), ("idepth", c_float_p), ("iR", c_float_p), ("my_type", c_float_p), ("status", c_u8_p)]


class InitPoints(C.Structure):
    """sdso_init_points_t: firstFrame->pointHessians after initializeFromInitializer STEP 3 (FullSystem.cpp:1533-1573)."""
    _fields_ = [("n", C.c_int), ("pnt", c_int_p), ("u", c_float_p), ("v", c_float_p), ("my_type", c_float_p), ("idepth", c_float_p), ("idepth_min", c_float_p),
                ("idepth_max", c_float_p), ("energyTH", c_float_p), ("color", c_float_p), ("weights", c_float_p)]


IMM_MAX_HOSTS = 8
IMM_NCOUNTS = 10   # lastTraceStatus histogram [0..5], forward GOOD, stereo outliers, intervals updated, unreadable


IMM_MATCH_NCOUNTS = 8   # walked, forward GOOD, back traces run, back GOOD, accepted, |du| >= 1, depth outside (0, max_depth), unreadable


class ImmMatchOut(C.Structure):
    """sdso_imm_match_out_t: the per-point results of sdso_imm_stereo_match and its dense map (FullSystem.cpp:598-611)."""
    _fields_ = [("accepted", c_u8_p), ("idepth", c_float_p), ("status_fwd", c_u8_p), ("status_back", c_u8_p), ("map", c_float_p)]


IMM_ACT_NCOUNTS = 17   # candidates, KEEP / DELETE / SELECT, toOptimize.size(), statuses -1 / 0 / 1, removed, the new count of every frame's group


class ImmActivate(C.Structure):
    """sdso_imm_activate_t: activatePointsMT STEP 2-5 on the resident set (FullSystem.cpp:837-957)."""
    _fields_ = [("nf", C.c_int), ("host_id", c_int_p), ("frame_slot", c_int_p), ("host_flagged", c_u8_p), ("geom", C.c_void_p),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_aff", c_float_p), ("w", C.c_int), ("h", C.c_int), ("K", C.c_float * 4),
                ("minObs", C.c_int), ("currentMinActDist", C.c_float), ("minTraceQuality", C.c_float)]


class ImmActivated(C.Structure):
    """sdso_imm_activated_t: one entry per selected candidate, in toOptimize order."""
    _fields_ = [("n", C.c_int), ("nf", C.c_int), ("frame", c_int_p), ("index", c_int_p), ("status", C.POINTER(C.c_int8)), ("idepth", c_float_p),
                ("res_state", c_u8_p), ("u", c_float_p), ("v", c_float_p), ("my_type", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("energyTH", c_float_p), ("color", c_float_p), ("weights", c_float_p), ("lastTraceStatus", c_u8_p)]


class Activate(C.Structure):
    _fields_ = [("nf", C.c_int), ("w", C.c_int), ("h", C.c_int), ("n", C.c_int), ("minObs", C.c_int), ("K", C.c_float * 4),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_aff", c_float_p), ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("host", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("energyTH", c_float_p)]


class DistMapGeom(C.Structure):
    """sdso_distmap_geom_t: K[1] * R * Ki[0] and K[1] * t of one keyframe into the newest (CoarseTracker.cpp:1235-1236)."""
    _fields_ = [("KRKi", C.c_float * 9), ("Kt", C.c_float * 3)]


class ActivateSelect(C.Structure):
    """sdso_activate_select_t: the candidates of FullSystem::activatePointsMT STEP 2 (FullSystem.cpp:837-902)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("ngeom", C.c_int), ("geom", C.POINTER(DistMapGeom)), ("host_flagged", c_u8_p),
                ("n", C.c_int), ("point_geom", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("quality", c_float_p), ("lastTracePixelInterval", c_float_p), ("lastTraceStatus", c_u8_p), ("my_type", c_float_p),
                ("currentMinActDist", C.c_float), ("minTraceQuality", C.c_float)]


def make_distmap_geoms(KRKi, Kt):
    """(ng, 3, 3) and (ng, 3) float32 arrays -> a ctypes array of DistMapGeom."""
    KRKi = np.ascontiguousarray(KRKi, np.float32).reshape(-1, 9)
    Kt = np.ascontiguousarray(Kt, np.float32).reshape(-1, 3)
    G = (DistMapGeom * max(1, len(KRKi)))()
    for g in range(len(KRKi)):
        G[g].KRKi[:] = KRKi[g].tolist()
        G[g].Kt[:] = Kt[g].tolist()
    return G


class StereoMatch(C.Structure):
    _fields_ = [("n", C.c_int), ("u", c_float_p), ("v", c_float_p), ("idepth_min_stereo", c_float_p), ("idepth_max_stereo", c_float_p),
                ("back_idepth_min_stereo", c_float_p), ("back_idepth_max_stereo", c_float_p), ("status_fwd", c_u8_p), ("status_back", c_u8_p),
                ("idepth_stereo", c_float_p), ("idepth_min_out", c_float_p), ("idepth_max_out", c_float_p), ("fwd_uv", c_float_p),
                ("back_uv", c_float_p)]


class G2oTrackEval(C.Structure):
    """sdso_g2o_track_eval_t: one EdgeSE3PosePhotoDSO evaluation point (fork-live tracker, dso_g2o_edge.cpp:395-500)."""
    _fields_ = [("lvl", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Ki", C.c_float * 9), ("RKi", C.c_float * 9), ("t_cull", C.c_float * 3),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("ab", C.c_float * 2), ("b0", C.c_double),
                ("cutoffTH", C.c_float), ("huberTH", C.c_float)]


class G2oLba(C.Structure):
    """sdso_g2o_lba_t: EdgeLBASE3PosePhotoIdepthCamDSO batch (dso_g2o_edge.cpp:5-282)."""
    _fields_ = [("nf", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_ab", c_float_p), ("host_b0", c_double_p),
                ("frameEnergyTH", c_float_p), ("cam", C.c_double * 4), ("host", c_int_p), ("target", c_int_p),
                ("u", c_float_p), ("v", c_float_p), ("idepth", c_double_p), ("color", c_float_p), ("weights", c_float_p)]


class G2oLbaWindow(C.Structure):
    """sdso_g2o_lba_window_t: the window graph of FullSystem::optimize, fork-live (FullSystemOptimize.cpp:455-542)."""
    _fields_ = [("nf", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("frame_slot", c_int_p), ("Ttw", C.POINTER(SE3)), ("target_aff", C.POINTER(Aff)), ("ab_exposure", c_float_p),
                ("host_b0", c_double_p), ("frameEnergyTH", c_float_p), ("host", c_int_p), ("target", c_int_p),
                ("u", c_float_p), ("v", c_float_p), ("color", c_float_p), ("weights", c_float_p)]


class G2oLbaState(C.Structure):
    """sdso_g2o_lba_state_t: the vertex estimates, in and out."""
    _fields_ = [("Twh", C.POINTER(SE3)), ("host_aff", C.POINTER(Aff)), ("cam", C.c_double * 4), ("idepth", c_double_p)]


class G2oLbaOpt(C.Structure):
    """sdso_g2o_lba_opt_t"""
    _fields_ = [("max_iterations", C.c_int), ("lambda_init", C.c_double), ("gain_threshold", C.c_double), ("max_trials", C.c_int)]


G2O_LBA_MAX_RECORDED = 64


class G2oLbaResult(C.Structure):
    """sdso_g2o_lba_result_t"""
    _fields_ = [("iterations", C.c_int), ("stop", C.c_int), ("n_active", C.c_int),
                ("trials", C.c_int * G2O_LBA_MAX_RECORDED), ("lambda_", C.c_double * G2O_LBA_MAX_RECORDED), ("chi2", C.c_double * G2O_LBA_MAX_RECORDED),
                ("chi2_final", C.c_double), ("rmse", C.c_float),
                ("state", c_u8_p), ("energy", c_float_p), ("centerProjectedTo", c_float_p), ("edge_level", c_u8_p),
                ("idepth_hessian", c_float_p), ("active", c_u8_p)]


class PoolStats(C.Structure):
    """sdso_pool_stats_t: the counters of a device buffer pool."""
    _fields_ = [(k, C.c_longlong) for k in ("hits", "misses", "frees", "host_waits", "overflow_waits", "parked_buffers", "parked_bytes")]


def fp(a):
    return a.ctypes.data_as(c_float_p)


def dp(a):
    return a.ctypes.data_as(c_double_p)


def ip(a):
    return a.ctypes.data_as(c_int_p)


def bp(a):
    return a.ctypes.data_as(c_u8_p)


def accum_floats(nf):
    return nf * nf * 91 * 2 + nf ** 3 * 64 + nf * nf * 32 + nf * nf * 8 + 16 + 4 + 2


def make_ba_window(win, frame_slots=None, dI_list=None):
    """Fill a BAWindow from the dict synth.ba_window() returns.  Keeps references alive in `keep`."""
    W = BAWindow()
    keep = []

    def arr(key, dt):
        a = np.ascontiguousarray(win[key], dtype=dt)
        keep.append(a)
        return a

    W.nf, W.np, W.nr, W.w, W.h = win["nf"], win["np"], win["nr"], win["w"], win["h"]
    W.calib_value_scaled[:] = list(win["calib_value_scaled"])
    W.calib_value_zero[:] = list(win["calib_value_zero"])
    W.evalPT = dp(arr("evalPT", np.float64))
    W.state = dp(arr("state", np.float64))
    W.state_zero = dp(arr("state_zero", np.float64))
    W.ab_exposure = fp(arr("ab_exposure", np.float32))
    W.frameEnergyTH = fp(arr("frameEnergyTH", np.float32))
    W.frameID = ip(arr("frameID", np.int32))
    if frame_slots is not None:
        fs = np.ascontiguousarray(frame_slots, np.int32)
        keep.append(fs)
        W.frame_slot = ip(fs)
    if dI_list is not None:
        ptrs = (c_float_p * len(dI_list))()
        for i, a in enumerate(dI_list):
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            ptrs[i] = fp(a)
        keep.append(ptrs)
        W.dI = C.cast(ptrs, C.POINTER(c_float_p))
    for key in ("u", "v", "idepth", "idepth_zero", "color", "weights"):
        setattr(W, key, fp(arr(key, np.float32)))
    W.host = ip(arr("host", np.int32))
    W.hasDepthPrior = bp(arr("hasDepthPrior", np.uint8))
    W.res_point = ip(arr("res_point", np.int32))
    W.res_target = ip(arr("res_target", np.int32))
    W.res_state = bp(arr("res_state", np.uint8))
    W.HM = dp(arr("HM", np.float64))
    W.bM = dp(arr("bM", np.float64))
    W.solverMode = int(win["solverMode"])
    W.affineOptModeA = float(win["affineOptModeA"])
    W.affineOptModeB = float(win["affineOptModeB"])
    W.forceAcceptStep = int(win["forceAcceptStep"])
    if win.get("maxRelBaseline") is not None:
        W.maxRelBaseline = fp(arr("maxRelBaseline", np.float32))
    if win.get("numGoodResiduals") is not None:
        W.numGoodResiduals = ip(arr("numGoodResiduals", np.int32))
    if win.get("res_isNew") is not None:
        W.res_isNew = bp(arr("res_isNew", np.uint8))
    return W, keep


def make_window_edit(drop_res=None, remove_points=None, drop_point=None, remove_frames=None, add_frames=None, add_res=None, add_points=None):
    """Fill a BAWindowEdit.  drop_res / remove_points / remove_frames: index sequences (their order is the order of the drops);
    drop_point: np flags; add_frames: dict(evalPT (k,12), state (k,10), state_zero (k,10), ab_exposure, frameEnergyTH, frameID,
    frame_slot); add_res: dict(point, target, state[, isNew]); add_points: dict(host, u, v, idepth, idepth_zero, color (k,8),
    weights (k,8), hasDepthPrior[, maxRelBaseline, numGoodResiduals], res_point, res_target, res_state[, res_isNew]).  Every index is in
    the numbering of the window before the call.  Returns (struct, keep-alive list)."""
    E = BAWindowEdit()
    keep = []
    conv = {np.float32: fp, np.float64: dp, np.int32: ip, np.uint8: bp}

    def put(field, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        setattr(E, field, conv[dt](a))
        return a

    if drop_res is not None:
        E.n_drop_res = len(put("drop_res", drop_res, np.int32))
    if remove_points is not None:
        E.n_remove_points = len(put("remove_points", remove_points, np.int32))
    if drop_point is not None:
        put("drop_point", drop_point, np.uint8)
    if remove_frames is not None:
        E.n_remove_frames = len(put("remove_frames", remove_frames, np.int32))
    if add_frames is not None:
        E.n_add_frames = len(put("frameID", add_frames["frameID"], np.int32))
        for k in ("evalPT", "state", "state_zero"):
            put(k, add_frames[k], np.float64)
        for k in ("ab_exposure", "frameEnergyTH"):
            put(k, add_frames[k], np.float32)
        put("frame_slot", add_frames["frame_slot"], np.int32)
    if add_res is not None:
        E.n_add_res = len(put("add_res_point", add_res["point"], np.int32))
        put("add_res_target", add_res["target"], np.int32)
        put("add_res_state", add_res["state"], np.uint8)
        if add_res.get("isNew") is not None:
            put("add_res_isNew", add_res["isNew"], np.uint8)
    if add_points is not None:
        E.n_add_points = len(put("pt_host", add_points["host"], np.int32))
        for k in ("u", "v", "idepth", "idepth_zero", "color", "weights"):
            put("pt_" + k, add_points[k], np.float32)
        put("pt_hasDepthPrior", add_points["hasDepthPrior"], np.uint8)
        if add_points.get("maxRelBaseline") is not None:
            put("pt_maxRelBaseline", add_points["maxRelBaseline"], np.float32)
        if add_points.get("numGoodResiduals") is not None:
            put("pt_numGoodResiduals", add_points["numGoodResiduals"], np.int32)
        E.n_pt_res = len(put("pt_res_point", add_points["res_point"], np.int32))
        put("pt_res_target", add_points["res_target"], np.int32)
        put("pt_res_state", add_points["res_state"], np.uint8)
        if add_points.get("res_isNew") is not None:
            put("pt_res_isNew", add_points["res_isNew"], np.uint8)
    return E, keep


def make_trace_points(n, u, v, color, weights, gradH, energyTH, idepth_min_stereo=None, idepth_max_stereo=None):
    """Fresh immature points (idepth_min=0, idepth_max=NaN; ImmaturePoint.cpp:34)."""
    d = dict(
        u_stereo=np.ascontiguousarray(u, np.float32).copy(), v_stereo=np.ascontiguousarray(v, np.float32).copy(),
        idepth_min=np.zeros(n, np.float32),
        idepth_min_stereo=(np.zeros(n, np.float32) if idepth_min_stereo is None else np.ascontiguousarray(idepth_min_stereo, np.float32).copy()),
        idepth_max_stereo=(np.full(n, np.nan, np.float32) if idepth_max_stereo is None else np.ascontiguousarray(idepth_max_stereo, np.float32).copy()),
        idepth_stereo=np.zeros(n, np.float32),
        color=np.ascontiguousarray(color, np.float32).copy(), weights=np.ascontiguousarray(weights, np.float32).copy(),
        gradH=np.ascontiguousarray(gradH, np.float32).copy(), energyTH=np.ascontiguousarray(energyTH, np.float32).copy(),
        quality=np.full(n, 10000, np.float32), lastTraceStatus=np.full(n, 5, np.uint8),
        lastTraceUV=np.zeros((n, 2), np.float32), lastTracePixelInterval=np.zeros(n, np.float32))
    P = TracePoints()
    P.n = n
    for k, a in d.items():
        setattr(P, k, bp(a) if a.dtype == np.uint8 else fp(a))
    return P, d


_lib = None


def load():
    """Load libsdso_hip.so (built by `make -C stereo-dso-g2o_amd/csrc` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsdso_hip.so is not built (%s): run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.sdso_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sdso_ctx_destroy.argtypes = [vp]
    L.sdso_ctx_destroy.restype = None
    L.sdso_last_error.argtypes = [vp]
    L.sdso_last_error.restype = C.c_char_p
    L.sdso_ctx_stream.argtypes = [vp]
    L.sdso_ctx_stream.restype = vp
    L.sdso_ctx_sync.argtypes = [vp]
    L.sdso_ctx_partition_cus.argtypes = [vp, C.c_int, C.c_int]
    L.sdso_prof_enable.argtypes = [vp, C.c_int]
    L.sdso_selftest_se3.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    L.sdso_prof_reset.argtypes = [vp]
    L.sdso_prof_read.argtypes = [vp, C.c_char_p, c_double_p, C.POINTER(C.c_long)]
    L.sdso_pyramid_levels.argtypes = [C.c_int, C.c_int]
    L.sdso_upload_pyramid.argtypes = [vp, C.c_int, C.c_int, c_int_p, c_int_p, C.POINTER(c_float_p)]
    L.sdso_make_pyramid.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_float_p]
    L.sdso_set_gamma.argtypes = [vp, c_float_p]
    L.sdso_gamma_from_binv.argtypes = [c_float_p, c_float_p]
    L.sdso_download_pyramid_level.argtypes = [vp, C.c_int, C.c_int, c_float_p]
    L.sdso_download_abs_grad.argtypes = [vp, C.c_int, C.c_int, c_float_p]
    L.sdso_release_pyramid.argtypes = [vp, C.c_int]
    L.sdso_track_set_ref.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]
    L.sdso_track_release_ref.argtypes = [vp, C.c_int]
    L.sdso_track_make_eval.argtypes = [C.POINTER(TrackParams), C.c_int, C.POINTER(SE3), C.POINTER(Aff), C.c_float, C.POINTER(TrackEval)]
    L.sdso_track_calc_res_gs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TrackEval), c_double_p, c_double_p, c_double_p, c_int_p, c_u8_p]
    L.sdso_track_calc_res_gs_batch.argtypes = [vp, C.c_int, c_int_p, c_int_p, C.POINTER(TrackEval), c_double_p, c_double_p, c_double_p, c_int_p]
    L.sdso_track_batch_prepare.argtypes = [vp, C.c_int, c_int_p, c_int_p, C.POINTER(TrackEval)]
    L.sdso_track_batch_enqueue.argtypes = [vp]
    L.sdso_track_batch_fetch.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_int_p]
    L.sdso_track_newest_coarse.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TrackParams), C.POINTER(SE3), C.POINTER(Aff), C.POINTER(TrackResult)]
    L.sdso_ba_upload_window.argtypes = [vp, C.c_int, C.POINTER(BAWindow)]
    L.sdso_ba_release_window.argtypes = [vp, C.c_int]
    L.sdso_ba_linearize.argtypes = [vp, C.c_int, c_double_p]
    L.sdso_ba_get_linearization.argtypes = [vp, C.c_int, c_float_p, c_u8_p, c_float_p, c_float_p, c_float_p, c_float_p]
    L.sdso_ba_apply_res.argtypes = [vp, C.c_int]
    L.sdso_ba_get_residual_state.argtypes = [vp, C.c_int, c_u8_p, c_u8_p, c_float_p]
    L.sdso_ba_get_ef_jacobians.argtypes = [vp, C.c_int, c_float_p]
    L.sdso_ba_accumulate.argtypes = [vp, C.c_int]
    L.sdso_ba_accum_floats.argtypes = [C.c_int]
    L.sdso_ba_accum_dev.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.sdso_ba_get_accumulators.argtypes = [vp, C.c_int, c_float_p]
    L.sdso_ba_set_accumulators.argtypes = [vp, C.c_int, c_float_p]
    L.sdso_ba_get_point_terms.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]
    L.sdso_ba_solve.argtypes = [vp, C.c_int, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.sdso_ba_get_point_steps.argtypes = [vp, C.c_int, c_float_p]
    L.sdso_ba_resubstitute.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p]
    L.sdso_ba_optimize.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_float_p, c_u8_p, C.POINTER(BAOptResult)]
    L.sdso_ba_marginalize_points.argtypes = [vp, C.c_int, c_u8_p, c_double_p, c_double_p]
    L.sdso_ba_get_tables.argtypes = [vp, C.c_int, c_float_p, c_double_p, c_double_p, c_float_p]
    L.sdso_ba_keep_projections.argtypes = [vp, C.c_int, C.c_int]
    L.sdso_ba_batch_create.argtypes = [vp, C.c_int, c_int_p]
    L.sdso_ba_batch_accumulate.argtypes = [vp]
    L.sdso_ba_batch_linearize.argtypes = [vp]
    L.sdso_ba_batch_schur.argtypes = [vp]
    L.sdso_ba_batch_set_materialize.argtypes = [vp, C.c_int]
    L.sdso_ba_batch_solve.argtypes = [vp, C.c_double, C.c_int]
    L.sdso_ba_batch_accum_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_long)]
    L.sdso_ba_batch_get_x.argtypes = [vp, c_double_p]
    L.sdso_ba_batch_optimize.argtypes = [vp, C.c_int, C.POINTER(BAOptResult)]
    L.sdso_ba_batch_optimize_begin.argtypes = [vp, C.c_int]
    L.sdso_ba_batch_step.argtypes = [vp]
    L.sdso_ba_batch_solve_step.argtypes = [vp, C.c_double, C.c_int]
    L.sdso_ba_batch_optimize_end.argtypes = [vp, C.POINTER(BAOptResult)]
    L.sdso_ba_get_state.argtypes = [vp, C.c_int, c_double_p, c_float_p, c_u8_p]
    L.sdso_ba_get_post_state.argtypes = [vp, C.c_int, C.POINTER(BAPostState)]
    L.sdso_ba_batch_keep_system.argtypes = [vp, C.c_int]
    L.sdso_ba_get_stitched.argtypes = [vp, C.c_int] + [c_double_p] * 6
    L.sdso_ba_batch_exchange_mode.argtypes = [vp, C.c_int]
    L.sdso_ba_get_counts.argtypes = [vp, C.c_int, c_int_p, c_int_p, c_int_p]
    L.sdso_ba_calc_energies.argtypes = [vp, C.c_int, c_double_p, c_double_p]
    L.sdso_ba_marginalize_frame_dev.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p]
    L.sdso_ba_adopt_prior.argtypes = [vp, C.c_int, C.c_int]
    L.sdso_ba_window_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, C.POINTER(BAWindowEdit), c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]
    L.sdso_ba_window_update.argtypes = [vp, C.c_int, C.POINTER(BAWindowEdit)]
    L.sdso_ba_window_get_order.argtypes = [vp, C.c_int, c_int_p, c_int_p, c_int_p]
    L.sdso_ba_window_update_activated.argtypes = [vp, C.c_int, C.POINTER(BAWindowEdit), c_int_p, c_int_p, c_int_p, c_int_p]
    L.sdso_ba_flag_points.argtypes = [vp, C.c_int, C.POINTER(BAFlagPoints), c_u8_p, c_int_p, c_int_p]
    L.sdso_ba_get_deltas.argtypes = [vp, C.c_int, c_float_p, c_double_p, c_double_p, c_float_p]
    L.sdso_comm_unique_id.argtypes = [vp]
    L.sdso_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.sdso_comm_attach.argtypes = [vp, vp]
    L.sdso_comm_init_host.argtypes = [vp, C.c_int, C.c_int, HOST_ALLREDUCE_FN, HOST_ALLGATHER_FN, vp]
    L.sdso_comm_info.argtypes = [vp, c_int_p, c_int_p]
    L.sdso_comm_destroy.argtypes = [vp]
    L.sdso_ba_allreduce.argtypes = [vp]
    L.sdso_ba_allreduce_window.argtypes = [vp, C.c_int]
    L.sdso_immature_init_batch.argtypes = [vp, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]
    L.sdso_trace_stereo_batch.argtypes = [vp, C.c_int, c_float_p, C.c_float, C.c_int, C.POINTER(TracePoints), c_u8_p]
    L.sdso_trace_stereo_prepare.argtypes = [vp, C.c_int, c_float_p, C.c_float, C.c_int, C.POINTER(TracePoints)]
    L.sdso_trace_stereo_enqueue.argtypes = [vp]
    L.sdso_trace_stereo_fetch.argtypes = [vp, C.POINTER(TracePoints), c_u8_p]
    L.sdso_track_newest_coarse_batch.argtypes = [vp, C.c_int, c_int_p, c_int_p, C.POINTER(TrackParams), C.POINTER(SE3), C.POINTER(Aff), C.POINTER(TrackResult)]
    L.sdso_track_make_ref.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_float_p, c_float_p, c_int_p]
    L.sdso_track_get_ref.argtypes = [vp, C.c_int, C.c_int, c_int_p, c_float_p, c_float_p, c_float_p, c_float_p]
    L.sdso_track_make_ref_from_window.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, c_int_p, C.c_int, c_int_p, c_int_p, c_int_p]
    L.sdso_track_get_ref_points.argtypes = [vp, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_float_p, c_u8_p, c_u8_p, c_float_p, c_float_p]
    L.sdso_trace_on_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TraceGeom), c_int_p, C.POINTER(TracePoints), c_u8_p]
    L.sdso_pixel_select.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.c_float, c_int_p, c_float_p, c_int_p]
    L.sdso_pixel_selector_pattern.argtypes = [C.c_int, c_u8_p]
    L.sdso_ba_marginalize_frame.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.sdso_activate_points_batch.argtypes = [vp, C.POINTER(Activate), C.POINTER(C.c_int8), c_float_p, c_u8_p]
    L.sdso_stereo_match_batch.argtypes = [vp, C.c_int, C.c_int, c_float_p, C.c_float, C.c_int, C.POINTER(StereoMatch)]
    L.sdso_g2o_track_add_edges.argtypes = [vp, C.c_int, C.c_int, C.POINTER(G2oTrackEval), c_double_p, c_int_p, c_u8_p, c_float_p]
    L.sdso_g2o_track_linearize.argtypes = [vp, C.c_int, C.c_int, C.POINTER(G2oTrackEval), c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.sdso_g2o_track_newest_coarse.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TrackParams), C.POINTER(SE3), C.POINTER(Aff), C.POINTER(TrackResult)]
    L.sdso_g2o_lba_eval.argtypes = [vp, C.POINTER(G2oLba), c_double_p, c_double_p, c_u8_p, c_float_p, c_float_p, c_float_p, c_u8_p]
    L.sdso_g2o_lba_optimize.argtypes = [vp, C.POINTER(G2oLbaWindow), C.POINTER(G2oLbaOpt), C.POINTER(G2oLbaState), C.POINTER(G2oLbaResult)]
    L.sdso_trace_set_gn_mode.argtypes = [vp, C.c_int]
    L.sdso_distmap_make.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(DistMapGeom), C.c_int, c_int_p, c_float_p, c_float_p, c_float_p, c_int_p]
    L.sdso_distmap_make_from_window.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(DistMapGeom), c_u8_p, c_int_p]
    L.sdso_distmap_add.argtypes = [vp, C.c_int, c_int_p, c_int_p]
    L.sdso_distmap_get.argtypes = [vp, c_float_p]
    L.sdso_activate_select.argtypes = [vp, C.POINTER(ActivateSelect), c_u8_p, c_int_p, c_int_p, c_int_p]
    L.sdso_undistort_make_remap.argtypes = [C.c_int, c_double_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_double_p, c_float_p, c_float_p, c_int_p]
    L.sdso_ingest_calib_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, c_float_p, c_float_p, C.c_int, C.c_int]
    L.sdso_ingest_calib_release.argtypes = [vp, C.c_int]
    L.sdso_ingest_frame.argtypes = [vp, C.c_int, C.c_int, c_int_p, C.POINTER(vp), c_float_p, C.c_float, c_float_p]
    L.sdso_init_set_first_stereo.argtypes = [vp, C.c_int, C.c_int, c_float_p, C.c_float, c_float_p, c_int_p, c_int_p]
    L.sdso_init_get_pnts.argtypes = [vp, C.POINTER(InitPnts)]
    L.sdso_init_from_initializer.argtypes = [vp, c_u8_p, c_int_p, c_int_p]
    L.sdso_init_get_points.argtypes = [vp, C.POINTER(InitPoints)]
    L.sdso_init_release.argtypes = [vp]
    L.sdso_imm_add_frame.argtypes = [vp, C.c_int, C.c_int, c_float_p, c_int_p]
    L.sdso_imm_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(ImmGeom), c_float_p, c_float_p, C.c_float, c_int_p]
    L.sdso_imm_count.argtypes = [vp, C.c_int, c_int_p]
    L.sdso_imm_get.argtypes = [vp, C.c_int, C.POINTER(TracePoints), c_float_p]
    L.sdso_imm_remove_order.argtypes = [C.c_int, c_u8_p, c_int_p, c_int_p]
    L.sdso_imm_remove.argtypes = [vp, C.c_int, C.c_int, c_u8_p]
    L.sdso_imm_release_host.argtypes = [vp, C.c_int]
    L.sdso_imm_put_host.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(TracePoints), c_float_p]
    L.sdso_imm_stereo_match.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_float_p, C.c_float, C.c_float, C.c_int, C.POINTER(ImmMatchOut), c_int_p]
    L.sdso_imm_stereo_match_fetch.argtypes = [vp, C.POINTER(ImmMatchOut), c_int_p]
    L.sdso_imm_stereo_map_dev.argtypes = [vp, C.POINTER(vp), c_int_p, c_int_p]
    L.sdso_imm_activate.argtypes = [vp, C.POINTER(ImmActivate), c_int_p]
    L.sdso_track_keep_depth_map.argtypes = [vp, C.c_int]
    L.sdso_track_depth_image.argtypes = [vp, C.c_int, C.c_int, c_float_p, c_float_p, c_u8_p, c_float_p, c_int_p]
    L.sdso_track_depth_image_dev.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), c_int_p, c_int_p]
    L.sdso_imm_activate_fetch.argtypes = [vp, C.POINTER(ImmActivated), c_u8_p]
    L.sdso_map_update.argtypes = [vp, C.c_int, C.POINTER(MapUpdate)]
    L.sdso_map_counts.argtypes = [vp, C.c_int, c_int_p]
    L.sdso_map_get.argtypes = [vp, C.c_int, C.c_int, c_float_p]
    L.sdso_map_put.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_float_p]
    L.sdso_map_release_keyframe.argtypes = [vp, C.c_int]
    L.sdso_map_clear.argtypes = [vp]
    L.sdso_map_cloud.argtypes = [vp, C.POINTER(MapCloud), c_float_p, c_u8_p, c_int_p, c_int_p]
    L.sdso_map_cloud_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), c_int_p]
    L.sdso_pyramid_export.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.sdso_pyramid_import.argtypes = [vp, C.c_int, vp]
    L.sdso_track_export_ref.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.sdso_track_import_ref.argtypes = [vp, C.c_int, vp]
    L.sdso_shared_info.argtypes = [vp, c_int_p, c_int_p, c_int_p]
    L.sdso_shared_release.argtypes = [vp]
    L.sdso_shared_release.restype = None
    L.sdso_shared_debug_buffers.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), c_int_p]
    L.sdso_pool_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(vp)]
    L.sdso_ctx_set_pool.argtypes = [vp, vp]
    L.sdso_pool_stats.argtypes = [vp, C.POINTER(PoolStats)]
    L.sdso_pool_trim.argtypes = [vp, C.c_size_t]
    L.sdso_pool_release.argtypes = [vp]
    L.sdso_pool_release.restype = None
    L.sdso_track_tries_replay.argtypes = [C.c_int, C.POINTER(SE3), C.POINTER(Aff), C.POINTER(TrackTry), c_double_p, C.c_double, C.POINTER(TrackTriesResult)]
    L.sdso_track_new_coarse.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TrackParams), C.c_int, C.POINTER(SE3), C.POINTER(Aff), c_double_p, C.c_double,
                                        C.POINTER(TrackTriesResult), C.POINTER(TrackTry)]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "sdso_ctx_create", "sdso_ctx_destroy", "sdso_last_error", "sdso_ctx_stream", "sdso_ctx_sync", "sdso_ctx_partition_cus",
    "sdso_prof_enable", "sdso_prof_reset", "sdso_prof_read", "sdso_selftest_se3",
    "sdso_pyramid_levels", "sdso_upload_pyramid", "sdso_make_pyramid", "sdso_set_gamma", "sdso_gamma_from_binv", "sdso_download_pyramid_level", "sdso_download_abs_grad",
    "sdso_release_pyramid", "sdso_track_set_ref", "sdso_track_release_ref", "sdso_track_make_eval",
    "sdso_track_calc_res_gs", "sdso_track_calc_res_gs_batch", "sdso_track_batch_prepare",
    "sdso_track_batch_enqueue", "sdso_track_batch_fetch", "sdso_track_newest_coarse",
    "sdso_ba_upload_window", "sdso_ba_release_window", "sdso_ba_linearize", "sdso_ba_get_linearization",
    "sdso_ba_apply_res", "sdso_ba_get_residual_state", "sdso_ba_get_ef_jacobians", "sdso_ba_accumulate", "sdso_ba_accum_floats",
    "sdso_ba_accum_dev", "sdso_ba_get_accumulators", "sdso_ba_set_accumulators", "sdso_ba_get_point_terms", "sdso_ba_solve",
    "sdso_ba_get_point_steps", "sdso_ba_optimize", "sdso_ba_marginalize_points", "sdso_ba_get_tables",
    "sdso_ba_keep_projections", "sdso_ba_batch_create", "sdso_ba_batch_accumulate", "sdso_ba_batch_solve",
    "sdso_ba_batch_accum_dev", "sdso_ba_batch_get_x", "sdso_ba_batch_set_materialize",
    "sdso_immature_init_batch", "sdso_trace_stereo_batch", "sdso_trace_stereo_prepare", "sdso_trace_stereo_enqueue",
    "sdso_trace_stereo_fetch", "sdso_stereo_match_batch", "sdso_activate_points_batch", "sdso_ba_marginalize_frame", "sdso_ba_batch_linearize", "sdso_ba_batch_schur", "sdso_pixel_select", "sdso_pixel_selector_pattern", "sdso_trace_on_batch", "sdso_track_make_ref", "sdso_track_newest_coarse_batch", "sdso_track_get_ref",
    "sdso_ba_get_post_state", "sdso_ba_batch_keep_system", "sdso_ba_get_stitched", "sdso_ba_batch_exchange_mode", "sdso_ba_resubstitute", "sdso_ba_get_counts", "sdso_ba_calc_energies", "sdso_ba_get_deltas", "sdso_ba_marginalize_frame_dev", "sdso_ba_adopt_prior",
    "sdso_ba_window_plan", "sdso_ba_window_update", "sdso_ba_window_update_activated", "sdso_ba_window_get_order",
    "sdso_ba_batch_optimize", "sdso_ba_batch_optimize_begin", "sdso_ba_batch_step", "sdso_ba_batch_solve_step", "sdso_ba_batch_optimize_end", "sdso_ba_get_state",
    "sdso_comm_unique_id", "sdso_comm_init", "sdso_comm_init_host", "sdso_comm_attach", "sdso_comm_info", "sdso_comm_destroy", "sdso_ba_allreduce", "sdso_ba_allreduce_window",
    "sdso_g2o_track_add_edges", "sdso_g2o_track_linearize", "sdso_g2o_track_newest_coarse", "sdso_g2o_lba_eval", "sdso_g2o_lba_optimize", "sdso_trace_set_gn_mode",
    "sdso_distmap_make", "sdso_distmap_make_from_window", "sdso_distmap_add", "sdso_distmap_get", "sdso_activate_select",
    "sdso_undistort_make_remap", "sdso_ingest_calib_create", "sdso_ingest_calib_release", "sdso_ingest_frame",
    "sdso_init_set_first_stereo", "sdso_init_get_pnts", "sdso_init_from_initializer", "sdso_init_get_points", "sdso_init_release",
    "sdso_imm_add_frame", "sdso_imm_trace", "sdso_imm_count", "sdso_imm_get", "sdso_imm_remove_order", "sdso_imm_remove", "sdso_imm_release_host",
    "sdso_imm_put_host", "sdso_imm_activate", "sdso_imm_activate_fetch",
    "sdso_imm_stereo_match", "sdso_imm_stereo_match_fetch", "sdso_imm_stereo_map_dev",
    "sdso_track_make_ref_from_window", "sdso_track_get_ref_points",
    "sdso_ba_flag_points",
    "sdso_track_keep_depth_map", "sdso_track_depth_image", "sdso_track_depth_image_dev",
    "sdso_map_update", "sdso_map_counts", "sdso_map_get", "sdso_map_put", "sdso_map_release_keyframe", "sdso_map_clear",
    "sdso_map_cloud", "sdso_map_cloud_dev",
    "sdso_pyramid_export", "sdso_pyramid_import", "sdso_track_export_ref", "sdso_track_import_ref", "sdso_shared_info", "sdso_shared_release",
    "sdso_shared_debug_buffers",
    "sdso_pool_create", "sdso_ctx_set_pool", "sdso_pool_stats", "sdso_pool_trim", "sdso_pool_release",
    "sdso_track_tries_replay", "sdso_track_new_coarse",
]


class SdsoError(RuntimeError):
    pass


class Shared:
    """One reference to an exported block of level buffers (sdso_shared); release() drops it."""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def info(self):
        """-> (kind: 0 pyramid / 1 template, device, holders: slots + handles)"""
        k, d, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        if self.L.sdso_shared_info(self.h, C.byref(k), C.byref(d), C.byref(n)) != 0:
            raise SdsoError("sdso_shared_info on a released handle")
        return k.value, d.value, n.value

    def release(self):
        if self.h:
            self.L.sdso_shared_release(self.h)
            self.h = None


class Pool:
    """The caller's reference to a device buffer pool (sdso_pool); release() drops it.  Attach ctxs with Context.set_pool."""

    def __init__(self, device=0, max_parked_bytes=1 << 30):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.sdso_pool_create(device, max_parked_bytes, C.byref(h))
        if rc != 0:
            raise SdsoError("sdso_pool_create(%d) failed with %d" % (device, rc))
        self.h = h

    def stats(self):
        """sdso_pool_stats -> dict of the counters"""
        st = PoolStats()
        if self.L.sdso_pool_stats(self.h, C.byref(st)) != 0:
            raise SdsoError("sdso_pool_stats on a released pool")
        return {k: getattr(st, k) for k, _ in PoolStats._fields_}

    def trim(self, keep_bytes=0):
        if self.L.sdso_pool_trim(self.h, keep_bytes) != 0:
            raise SdsoError("sdso_pool_trim on a released pool")

    def release(self):
        if self.h:
            self.L.sdso_pool_release(self.h)
            self.h = None


class Context:
    """One GPU + one HIP stream (sdso_ctx)."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.sdso_ctx_create(device, C.byref(h))
        if rc != 0:
            raise SdsoError("sdso_ctx_create(%d) failed with %d: no usable HIP device (no CPU fallback)" % (device, rc))
        self.h = h

    def check(self, rc):
        if rc != 0:
            msg = self.L.sdso_last_error(self.h)
            raise SdsoError("sdso call failed (%d): %s" % (rc, msg.decode() if msg else ""))

    def close(self):
        if self.h:
            self.L.sdso_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self.check(self.L.sdso_ctx_sync(self.h))

    def prof_read(self, kernel):
        ms = C.c_double(0)
        n = C.c_long(0)
        self.check(self.L.sdso_prof_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def ingest_frame(self, calib, slots, raws, exposure, factor=1.0):
        """sdso_ingest_frame for 1 or 2 raw images (uint8 / uint16 arrays); enqueue-only.  Returns exposure_out."""
        n = len(slots)
        arrs = [np.ascontiguousarray(r) for r in raws]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        ex = np.ascontiguousarray(exposure, np.float32)
        out = np.zeros(n, np.float32)
        self.check(self.L.sdso_ingest_frame(self.h, calib, n, (C.c_int * n)(*slots), ptrs, fp(ex), factor, fp(out)))
        return out

    def init_set_first_stereo(self, frame_slot, right_slot, K4, baseline, selection_map=None, read=True):
        """sdso_init_set_first_stereo -> (numPoints[0], counts); read=False: the enqueue-only form -> (None, None)."""
        K = np.ascontiguousarray(K4, np.float32)
        m = None if selection_map is None else np.ascontiguousarray(selection_map, np.float32)
        n = C.c_int(-1)
        counts = np.full(INIT_NCOUNTS, -1, np.int32)
        self.check(self.L.sdso_init_set_first_stereo(self.h, frame_slot, right_slot, fp(K), baseline, None if m is None else fp(m),
                                                     C.byref(n) if read else None, ip(counts) if read else None))
        return (n.value, counts) if read else (None, None)

    def init_get_pnts(self, cap):
        """sdso_init_get_pnts into arrays of cap entries -> dict of the Pnt members, cut to the n the library set."""
        d = dict(u=np.full(cap, -1, np.float32), v=np.full(cap, -1, np.float32), idepth=np.full(cap, -1, np.float32), iR=np.full(cap, -1, np.float32),
                 my_type=np.full(cap, -1, np.float32), status=np.full(cap, 254, np.uint8))
        P = InitPnts()
        P.n = -1
        for k, a in d.items():
            setattr(P, k, bp(a) if a.dtype == np.uint8 else fp(a))
        self.check(self.L.sdso_init_get_pnts(self.h, C.byref(P)))
        assert 0 <= P.n <= cap
        return {k: a[:P.n] for k, a in d.items()}

    def init_from_initializer(self, keep=None, read=True):
        """sdso_init_from_initializer -> (points made, counts); read=False: the enqueue-only form -> (None, None)."""
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        n = C.c_int(-1)
        counts = np.full(4, -1, np.int32)
        self.check(self.L.sdso_init_from_initializer(self.h, None if k is None else bp(k), C.byref(n) if read else None, ip(counts) if read else None))
        return (n.value, counts) if read else (None, None)

    def init_get_points(self, cap):
        """sdso_init_get_points into arrays of cap entries -> dict of the PointHessian records, cut to the n the library set."""
        d = dict(pnt=np.full(cap, -1, np.int32))
        d.update({k: np.full(cap, -1, np.float32) for k in ("u", "v", "my_type", "idepth", "idepth_min", "idepth_max", "energyTH")})
        d.update(color=np.full((cap, 8), -1, np.float32), weights=np.full((cap, 8), -1, np.float32))
        P = InitPoints()
        P.n = -1
        for k, a in d.items():
            setattr(P, k, ip(a) if a.dtype == np.int32 else fp(a))
        self.check(self.L.sdso_init_get_points(self.h, C.byref(P)))
        assert 0 <= P.n <= cap
        return {k: a[:P.n] for k, a in d.items()}

    def imm_get(self, host_id):
        """sdso_imm_get: one host's immature points as a dict of numpy arrays (the members of ImmaturePoint, in the set's order)."""
        n = C.c_int(0)
        self.check(self.L.sdso_imm_count(self.h, host_id, C.byref(n)))
        n = n.value
        P, d = make_trace_points(n, np.zeros(n), np.zeros(n), np.zeros((n, 8)), np.zeros((n, 8)), np.zeros((n, 4)), np.zeros(n))
        P.idepth_min = None; P.idepth_stereo = None
        my_type = np.zeros(n, np.float32)
        self.check(self.L.sdso_imm_get(self.h, host_id, C.byref(P), fp(my_type)))
        assert P.n == n
        return dict(u=d["u_stereo"], v=d["v_stereo"], my_type=my_type, idepth_min=d["idepth_min_stereo"], idepth_max=d["idepth_max_stereo"],
                    quality=d["quality"], color=d["color"], weights=d["weights"], gradH=d["gradH"], energyTH=d["energyTH"],
                    lastTraceStatus=d["lastTraceStatus"], lastTraceUV=d["lastTraceUV"], lastTracePixelInterval=d["lastTracePixelInterval"])

    def imm_put(self, host_id, S, w, h):
        """sdso_imm_put_host: installs a group from a dict of arrays as imm_get returns it."""
        n = len(S["u"])
        a = {k: np.ascontiguousarray(S[k], np.uint8 if k == "lastTraceStatus" else np.float32) for k in
             ("u", "v", "my_type", "idepth_min", "idepth_max", "quality", "color", "weights", "gradH", "energyTH", "lastTraceStatus", "lastTraceUV",
              "lastTracePixelInterval")}
        P = TracePoints()
        P.n = n
        P.u_stereo = fp(a["u"]); P.v_stereo = fp(a["v"]); P.idepth_min_stereo = fp(a["idepth_min"]); P.idepth_max_stereo = fp(a["idepth_max"])
        for k in ("color", "weights", "gradH", "energyTH", "quality", "lastTraceUV", "lastTracePixelInterval"):
            setattr(P, k, fp(a[k]))
        P.lastTraceStatus = bp(a["lastTraceStatus"])
        self.check(self.L.sdso_imm_put_host(self.h, host_id, w, h, C.byref(P), fp(a["my_type"])))

    def imm_match_arrays(self, n, w=0, h=0, statuses=True):
        """An ImmMatchOut over fresh arrays for n points (and a w x h map where w > 0) -> (struct, dict of the arrays, counts)."""
        d = dict(accepted=np.full(n, 255, np.uint8), idepth=np.full((n, 3), -1, np.float32))
        if statuses:
            d.update(status_fwd=np.full(n, 254, np.uint8), status_back=np.full(n, 254, np.uint8))
        if w > 0:
            d["map"] = np.full((h, w, 3), -1, np.float32)
        O = ImmMatchOut()
        for k, a in d.items():
            setattr(O, k, bp(a) if a.dtype == np.uint8 else fp(a))
        return O, d, np.full(IMM_MATCH_NCOUNTS, -1, np.int32)

    def imm_stereo_match(self, host_id, frame_slot, right_slot, K4, baseline, max_depth=70.0, map_wh=None, statuses=True):
        """sdso_imm_stereo_match: stereoMatch's loop (FullSystem.cpp:581-613) on one group -> dict of arrays: accepted, idepth [n, 3],
        status_fwd, status_back, counts and, with map_wh = (w, h) of the group's image, map [h, w, 3]."""
        n = C.c_int(0)
        self.check(self.L.sdso_imm_count(self.h, host_id, C.byref(n)))
        w, h = map_wh if map_wh else (0, 0)
        O, d, counts = self.imm_match_arrays(n.value, w, h, statuses)
        K = np.ascontiguousarray(K4, np.float32)
        self.check(self.L.sdso_imm_stereo_match(self.h, host_id, frame_slot, right_slot, fp(K), baseline, max_depth, 1 if map_wh else 0, C.byref(O), ip(counts)))
        d["counts"] = counts
        return d

    def imm_stereo_match_fetch(self, n, w=0, h=0, statuses=True):
        """sdso_imm_stereo_match_fetch -> the dict of imm_stereo_match for the latest call (n its group's count; a map where w > 0)."""
        O, d, counts = self.imm_match_arrays(n, w, h, statuses)
        self.check(self.L.sdso_imm_stereo_match_fetch(self.h, C.byref(O), ip(counts)))
        d["counts"] = counts
        return d

    def imm_stereo_map_dev(self):
        """sdso_imm_stereo_map_dev -> (device pointer, w, h)"""
        p, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
        self.check(self.L.sdso_imm_stereo_map_dev(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def imm_activate_raw(self, host_id, frame_slot, host_flagged, KRKi, Kt, pair_R, pair_t, pair_aff, w, h, K4, min_obs, min_act_dist, min_trace_quality=3.0):
        """sdso_imm_activate without the fetch -> (return code, counts)."""
        nf = len(host_id)
        keep = [np.ascontiguousarray(host_id, np.int32), np.ascontiguousarray(frame_slot, np.int32), np.ascontiguousarray(host_flagged, np.uint8),
                np.ascontiguousarray(pair_R, np.float32), np.ascontiguousarray(pair_t, np.float32), np.ascontiguousarray(pair_aff, np.float32)]
        G = make_distmap_geoms(KRKi, Kt)
        A = ImmActivate()
        A.nf = nf; A.host_id = ip(keep[0]); A.frame_slot = ip(keep[1]); A.host_flagged = bp(keep[2]); A.geom = C.cast(G, C.c_void_p)
        A.pair_R = fp(keep[3]); A.pair_t = fp(keep[4]); A.pair_aff = fp(keep[5])
        A.w, A.h, A.minObs, A.currentMinActDist, A.minTraceQuality = w, h, min_obs, min_act_dist, min_trace_quality
        A.K[:] = [float(x) for x in K4]
        counts = np.full(IMM_ACT_NCOUNTS, -1, np.int32)
        rc = self.L.sdso_imm_activate(self.h, C.byref(A), ip(counts))
        return rc, counts

    def imm_activate_fetch(self, n_candidates, n_selected, nf):
        """sdso_imm_activate_fetch -> dict of arrays (one entry per selected candidate) with `decision` (one per candidate)."""
        n = n_selected
        d = dict(frame=np.zeros(n, np.int32), index=np.zeros(n, np.int32), status=np.zeros(n, np.int8), idepth=np.zeros(n, np.float32),
                 res_state=np.zeros((n, nf), np.uint8), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), my_type=np.zeros(n, np.float32),
                 idepth_min=np.zeros(n, np.float32), idepth_max=np.zeros(n, np.float32), energyTH=np.zeros(n, np.float32),
                 color=np.zeros((n, 8), np.float32), weights=np.zeros((n, 8), np.float32), lastTraceStatus=np.zeros(n, np.uint8))
        O = ImmActivated()
        for k, a in d.items():
            setattr(O, k, a.ctypes.data_as(C.POINTER(C.c_int8)) if a.dtype == np.int8 else {np.dtype(np.float32): fp, np.dtype(np.int32): ip, np.dtype(np.uint8): bp}[a.dtype](a))
        dec = np.zeros(n_candidates, np.uint8)
        self.check(self.L.sdso_imm_activate_fetch(self.h, C.byref(O), bp(dec)))
        assert O.n == n and O.nf == nf
        d["decision"] = dec
        return d

    def imm_activate(self, host_id, *args, **kw):
        """sdso_imm_activate + sdso_imm_activate_fetch -> (counts, dict of the activated records)."""
        rc, counts = self.imm_activate_raw(host_id, *args, **kw)
        self.check(rc)
        return counts, self.imm_activate_fetch(int(counts[0]), int(counts[4]), len(host_id))

    def distmap_make_from_window(self, wid, w, h, KRKi, Kt, skip=None, count=True):
        """sdso_distmap_make_from_window -> (return code, n_seeds); count=False passes n_seeds = NULL (no synchronisation) -> (rc, None).
        KRKi = None passes a null geom."""
        G = None if KRKi is None else make_distmap_geoms(KRKi, Kt)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        n = C.c_int(-1)
        rc = self.L.sdso_distmap_make_from_window(self.h, wid, w, h, G, None if sk is None else bp(sk), C.byref(n) if count else None)
        return rc, (n.value if count else None)

    def window_update_activated(self, wid, E, act_frame, cap):
        """sdso_ba_window_update_activated with the BAWindowEdit E -> (return code, n_points, n_res, act_index); act_frame = None passes a
        null map; cap: entries act_index is sized for (counts[4] of the activation)."""
        af = None if act_frame is None else np.ascontiguousarray(act_frame, np.int32)
        n_pt, n_res = C.c_int(-1), C.c_int(-1)
        idx = np.full(max(1, cap), -1, np.int32)
        rc = self.L.sdso_ba_window_update_activated(self.h, wid, C.byref(E), None if af is None else ip(af), C.byref(n_pt), C.byref(n_res), ip(idx))
        return rc, n_pt.value, n_res.value, idx[:max(0, n_pt.value)]

    def flag_points(self, wid, nf, npts, frame_marg, last_gone=None, **settings):
        """sdso_ba_flag_points -> (decision [np], counts [6], host_counts [nf, 6])."""
        F, keep = make_flag_points(frame_marg, last_gone, **settings)
        dec, cnt, hc = np.full(npts, 255, np.uint8), np.full(6, -1, np.int32), np.full((nf, 6), -1, np.int32)
        self.check(self.L.sdso_ba_flag_points(self.h, wid, C.byref(F), bp(dec), ip(cnt), ip(hc)))
        return dec, cnt, hc

    def keep_depth_map(self, on=True):
        """sdso_track_keep_depth_map: templates built from now on keep their level-0 map."""
        self.check(self.L.sdso_track_keep_depth_map(self.h, 1 if on else 0))

    def depth_image_raw(self, ref_slot, frame_slot, w, h, prev=None, rgb=True, idepth=True):
        """sdso_track_depth_image without the check -> (return code, dict).  prev = (minID, maxID) stands for *minID_pt / *maxID_pt,
        None for two null pointers; dict: rgb [h, w, 3] uint8, idepth [h, w], counts [2], range (the two values after the call, or None)."""
        d = dict(counts=np.full(2, -1, np.int32))
        if rgb:
            d["rgb"] = np.full((h, w, 3), 77, np.uint8)
        if idepth:
            d["idepth"] = np.full((h, w), -7, np.float32)
        r = None if prev is None else np.array(prev, np.float32)
        rc = self.L.sdso_track_depth_image(self.h, ref_slot, frame_slot, None if r is None else fp(r[0:1]), None if r is None else fp(r[1:2]),
                                           bp(d["rgb"]) if rgb else None, fp(d["idepth"]) if idepth else None, ip(d["counts"]))
        d["range"] = None if r is None else (r[0], r[1])
        return rc, d

    def depth_image(self, ref_slot, frame_slot, w, h, prev=None, rgb=True, idepth=True):
        """sdso_track_depth_image (debugPlotIDepthMap / debugPlotIDepthMapFloat on the slot's kept map) -> the dict of depth_image_raw."""
        rc, d = self.depth_image_raw(ref_slot, frame_slot, w, h, prev, rgb, idepth)
        self.check(rc)
        return d

    def depth_image_dev(self, ref_slot):
        """sdso_track_depth_image_dev -> (rgb device pointer, idepth device pointer, w, h)"""
        a, b, w, h = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
        self.check(self.L.sdso_track_depth_image_dev(self.h, ref_slot, C.byref(a), C.byref(b), C.byref(w), C.byref(h)))
        return a.value, b.value, w.value, h.value

    def map_update_raw(self, wid, active, gone, gone_list):
        """sdso_map_update without the check -> return code.  active: window point indices or None (every point not in gone)."""
        U = MapUpdate()
        a = None if active is None else np.ascontiguousarray(active, np.int32)
        g, gl = np.ascontiguousarray(gone, np.int32), np.ascontiguousarray(gone_list, np.uint8)
        U.n_active = 0 if a is None else len(a)
        U.active = None if a is None else ip(a)
        U.n_gone = len(g); U.gone = ip(g); U.gone_list = bp(gl)
        return self.L.sdso_map_update(self.h, wid, C.byref(U))

    def map_update(self, wid, active, gone, gone_list):
        self.check(self.map_update_raw(wid, active, gone, gone_list))

    def map_counts(self, frame_id):
        """sdso_map_counts -> [active, marginalised, out]"""
        c = np.full(3, -1, np.int32)
        self.check(self.L.sdso_map_counts(self.h, frame_id, ip(c)))
        return c

    def map_get(self, frame_id, lst):
        """sdso_map_get -> records [n, 16] of list 1 (active), 2 (marginalised) or 3 (out)"""
        n = int(self.map_counts(frame_id)[lst - 1])
        r = np.full((n, MAP_REC_FLOATS), -9, np.float32)
        self.check(self.L.sdso_map_get(self.h, frame_id, lst, fp(r)))
        return r

    def map_put(self, frame_id, lst, records):
        r = np.ascontiguousarray(records, np.float32).reshape(-1, MAP_REC_FLOATS)
        self.check(self.L.sdso_map_put(self.h, frame_id, lst, len(r), fp(r)))

    def map_cloud_raw(self, frame_ids, K4, scaledTH=0.001, absTH=0.001, minBS=0.1, mode=1, imm_host_id=None, camToWorld=None, cap=None, bound=None):
        """sdso_map_cloud without the check -> (return code, dict: xyz [cap, 3], rgb [cap, 3] (untouched past n), first, kept [n_frames, 4], n).
        cap defaults to the bound 8 x the sum of the list sizes."""
        nfr = len(frame_ids)
        fid = np.ascontiguousarray(frame_ids, np.int32)
        imm = None if imm_host_id is None else np.ascontiguousarray(imm_host_id, np.int32)
        if cap is None:
            cap = 0
            for k in range(nfr):
                cap += 8 * int(self.map_counts(int(fid[k])).sum())
                if imm is not None and imm[k] >= 0:
                    n = C.c_int(0)
                    self.check(self.L.sdso_imm_count(self.h, int(imm[k]), C.byref(n)))
                    cap += 8 * n.value
        T = None if camToWorld is None else np.ascontiguousarray(camToWorld, np.float32)
        Q = MapCloud()
        Q.n_frames = nfr; Q.frameID = ip(fid); Q.imm_host_id = None if imm is None else ip(imm)
        Q.fx, Q.fy, Q.cx, Q.cy = [float(x) for x in K4]
        Q.scaledTH, Q.absTH, Q.minBS, Q.mode = scaledTH, absTH, minBS, mode
        Q.camToWorld = None if T is None else fp(T)
        Q.cap = cap
        d = dict(xyz=np.full((max(cap, 1), 3), -77, np.float32), rgb=np.full((max(cap, 1), 3), 77, np.uint8), first=np.full(nfr + 1, -1, np.int32),
                 kept=np.full((nfr, 4), -1, np.int32))
        rc = self.L.sdso_map_cloud(self.h, C.byref(Q), fp(d["xyz"]), bp(d["rgb"]), ip(d["first"]), ip(d["kept"]))
        d["n"] = int(d["first"][nfr])
        return rc, d

    def map_cloud(self, frame_ids, K4, **kw):
        """sdso_map_cloud -> the dict of map_cloud_raw"""
        rc, d = self.map_cloud_raw(frame_ids, K4, **kw)
        self.check(rc)
        return d

    def map_cloud_dev(self):
        """sdso_map_cloud_dev -> (xyz device pointer, rgb device pointer, n)"""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self.check(self.L.sdso_map_cloud_dev(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def read_device(self, ptr, nbytes):
        """nbytes at a device pointer of this context, after its stream has drained (hipMemcpy through the HIP runtime the library uses)"""
        self.sync()
        out = np.zeros(nbytes, np.uint8)
        rc = self.L.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2)   # hipMemcpyDeviceToHost
        if rc != 0:
            raise SdsoError("hipMemcpy from the device failed (%d)" % rc)
        return out

    def export_pyramid(self, frame_slot):
        """sdso_pyramid_export -> Shared (one more holder of the slot's level buffers)"""
        h = C.c_void_p()
        self.check(self.L.sdso_pyramid_export(self.h, frame_slot, C.byref(h)))
        return Shared(self.L, h)

    def import_pyramid(self, frame_slot, shared):
        self.check(self.L.sdso_pyramid_import(self.h, frame_slot, shared.h))

    def export_ref(self, ref_slot):
        """sdso_track_export_ref -> Shared"""
        h = C.c_void_p()
        self.check(self.L.sdso_track_export_ref(self.h, ref_slot, C.byref(h)))
        return Shared(self.L, h)

    def import_ref(self, ref_slot, shared):
        self.check(self.L.sdso_track_import_ref(self.h, ref_slot, shared.h))

    def set_pool(self, pool):
        """sdso_ctx_set_pool; None detaches"""
        self.check(self.L.sdso_ctx_set_pool(self.h, pool.h if pool is not None else None))

    def slot_buffers(self, kind, slot):
        """sdso_shared_debug_buffers -> (device addresses of the SDSO_PYR_LEVELS level buffers, is_view)"""
        a = (C.c_ulonglong * 6)()
        v = C.c_int(0)
        self.check(self.L.sdso_shared_debug_buffers(self.h, kind, slot, a, C.byref(v)))
        return list(a), bool(v.value)

    def upload_pyramid(self, slot, pyr):
        n = len(pyr)
        ws = (C.c_int * n)(*[p.shape[1] for p in pyr])
        hs = (C.c_int * n)(*[p.shape[0] for p in pyr])
        arrs = [np.ascontiguousarray(p, np.float32) for p in pyr]
        ptrs = (c_float_p * n)(*[fp(a) for a in arrs])
        self.check(self.L.sdso_upload_pyramid(self.h, slot, n, ws, hs, ptrs))

    def set_ref(self, ref_slot, pc):
        for lvl, p in enumerate(pc):
            u, v, i, c = [np.ascontiguousarray(p[k], np.float32) for k in ("u", "v", "idepth", "color")]
            self.check(self.L.sdso_track_set_ref(self.h, ref_slot, lvl, len(u), fp(u), fp(v), fp(i), fp(c)))
