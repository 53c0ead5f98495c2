"""The structures and constants of include/sdso_abi.h as ctypes sees them.

Every class names the C type it mirrors in _c_name_; tests/test_abi_layout_cpu.py compiles the header and holds each class to its
sizeof, member offsets and member sizes, and each typedef of the header to exactly one class here."""
import ctypes as C

import numpy as np

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_u8_p = C.POINTER(C.c_uint8)
c_i8_p = C.POINTER(C.c_int8)

C_MEMBER_NAMES = {"lambda_": "lambda"}   # the members whose C name is a Python keyword: ctypes name -> C name


class TrackEval(C.Structure):
    _c_name_ = "sdso_track_eval_t"
    _fields_ = [("lvl", C.c_int), ("w", C.c_int), ("h", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Ki", C.c_float * 9), ("RKi", C.c_float * 9), ("t", C.c_float * 3), ("affLL", C.c_float * 2), ("ref_b0", C.c_float),
                ("cutoffTH", C.c_float), ("huberTH", C.c_float)]


class SE3(C.Structure):
    _c_name_ = "sdso_se3_t"
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
    _c_name_ = "sdso_aff_t"
    _fields_ = [("a", C.c_double), ("b", C.c_double)]


class TrackParams(C.Structure):
    _c_name_ = "sdso_track_params_t"
    _fields_ = [("levels", C.c_int), ("w", C.c_int * 6), ("h", C.c_int * 6),
                ("fx", C.c_float * 6), ("fy", C.c_float * 6), ("cx", C.c_float * 6), ("cy", C.c_float * 6),
                ("ref_exposure", C.c_float), ("new_exposure", C.c_float), ("ref_aff_g2l", Aff), ("coarsestLvl", C.c_int), ("minResForAbort", C.c_double * 5),
                ("coarseCutoffTH", C.c_float), ("huberTH", C.c_float), ("maxIterations", C.c_int * 5),
                ("affineOptModeA", C.c_double), ("affineOptModeB", C.c_double)]


class TrackResult(C.Structure):
    _c_name_ = "sdso_track_result_t"
    _fields_ = [("good", C.c_int), ("lastResiduals", C.c_double * 5), ("lastFlowIndicators", C.c_double * 3),
                ("iterations", C.c_int * 5), ("evaluations", C.c_int), ("point_evals", C.c_longlong)]


class TrackTrace(C.Structure):
    """The finish_level events of one try."""
    _c_name_ = "sdso_track_trace_t"
    _fields_ = [("n", C.c_int), ("lvl", C.c_int * 6), ("res", C.c_double * 6), ("flow", (C.c_double * 3) * 6)]


class TrackTry(C.Structure):
    """One try of FullSystem::trackNewCoarse's loop — as it ran (trace, end_*) and as the loop saw it."""
    _c_name_ = "sdso_track_try_t"
    _fields_ = [("trace", TrackTrace), ("end_good", C.c_int), ("end_pose", SE3), ("end_aff", Aff),
                ("ran", C.c_int), ("good", C.c_int), ("abort_lvl", C.c_int), ("winner", C.c_int),
                ("lastResiduals", C.c_double * 5), ("lastFlowIndicators", C.c_double * 3), ("pose", SE3), ("aff", Aff)]


class TrackTriesResult(C.Structure):
    _c_name_ = "sdso_track_tries_result_t"
    _fields_ = [("haveOneGood", C.c_int), ("winner", C.c_int), ("tryIterations", C.c_int), ("pose", SE3), ("aff", Aff),
                ("flowVecs", C.c_double * 3), ("achievedRes", C.c_double * 5)]


class BAWindow(C.Structure):
    _c_name_ = "sdso_ba_window_t"
    _fields_ = [("nf", C.c_int), ("np", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("calib_value_scaled", C.c_double * 4), ("calib_value_zero", C.c_double * 4),
                ("evalPT", c_double_p), ("state", c_double_p), ("state_zero", c_double_p),
                ("ab_exposure", c_float_p), ("frameEnergyTH", c_float_p), ("frameID", c_int_p), ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("u", c_float_p), ("v", c_float_p), ("idepth", c_float_p), ("idepth_zero", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("host", c_int_p), ("hasDepthPrior", c_u8_p),
                ("res_point", c_int_p), ("res_target", c_int_p), ("res_state", c_u8_p), ("HM", c_double_p), ("bM", c_double_p),
                ("solverMode", C.c_int), ("affineOptModeA", C.c_double), ("affineOptModeB", C.c_double), ("forceAcceptStep", C.c_int),
                ("maxRelBaseline", c_float_p), ("numGoodResiduals", c_int_p), ("res_isNew", c_u8_p)]


class BAWindowEdit(C.Structure):
    """The seven stages of sdso_ba_window_update (include/sdso_abi.h)."""
    _c_name_ = "sdso_ba_window_edit_t"
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
    _c_name_ = "sdso_ba_opt_result_t"
    _fields_ = [("iterations", C.c_int), ("lastEnergy", C.c_double), ("rmse", C.c_double), ("resInA", C.c_int)]


class BAPostState(C.Structure):
    """What FullSystem::optimize leaves behind (FullSystemOptimize.cpp:52-87, :142-203, :997-1041)."""
    _c_name_ = "sdso_ba_post_state_t"
    _fields_ = [("idepth", c_float_p), ("step", c_float_p), ("HdiF", c_float_p), ("bdSumF", c_float_p), ("idepth_hessian", c_float_p),
                ("maxRelBaseline", c_float_p), ("numGoodResiduals", c_int_p),
                ("state_state", c_u8_p), ("isActiveAndIsGoodNEW", c_u8_p), ("state_energy", c_float_p), ("centerProjectedTo", c_float_p),
                ("projectedTo", c_float_p), ("toRemove", c_u8_p),
                ("state", c_double_p), ("state_zero", c_double_p), ("evalPT", c_double_p), ("PRE_worldToCam", c_double_p),
                ("frame_step", c_double_p), ("frameEnergyTH", c_float_p),
                ("calib_value", C.c_double * 4), ("calib_value_scaled", C.c_double * 4), ("calib_step", C.c_double * 4),
                ("lastX", c_double_p), ("lastHS", c_double_p), ("lastbS", c_double_p),
                ("resInA", C.c_int), ("resInL", C.c_int), ("resInM", C.c_int), ("n_toRemove", C.c_int), ("result", BAOptResult)]


PT_KEEP, PT_DROP_NO_RESIDUAL, PT_DROP_NEGATIVE, PT_MARGINALIZE, PT_DROP_WEAK, PT_DROP_NOT_INLIER = range(6)   # SDSO_PT_*


class BAFlagPoints(C.Structure):
    """removeOutliers + flagPointsForRemoval on the resident window (FullSystem.cpp:965-1056)."""
    _c_name_ = "sdso_ba_flag_points_t"
    _fields_ = [("frame_marg", c_u8_p), ("last_gone", c_u8_p), ("minGoodActiveResForMarg", C.c_int), ("minGoodResForMarg", C.c_int),
                ("minIdepthH_marg", C.c_float)]


class MapUpdate(C.Structure):
    """The orders of a keyframe's point lists (window point indices)."""
    _c_name_ = "sdso_map_update_t"
    _fields_ = [("n_active", C.c_int), ("active", c_int_p), ("n_gone", C.c_int), ("gone", c_int_p), ("gone_list", c_u8_p)]


class MapCloud(C.Structure):
    """KeyFrameDisplay::refreshPC for up to 8 keyframes."""
    _c_name_ = "sdso_map_cloud_t"
    _fields_ = [("n_frames", C.c_int), ("frameID", c_int_p), ("imm_host_id", c_int_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("scaledTH", C.c_float), ("absTH", C.c_float), ("minBS", C.c_float), ("mode", C.c_int), ("camToWorld", c_float_p),
                ("cap", C.c_int)]


MAP_REC_FLOATS = 16          # u, v, idepth, idepth_hessian, maxRelBaseline, color[8], padding (csrc/map_cloud.h)


class TracePoints(C.Structure):
    _c_name_ = "sdso_trace_points_t"
    _fields_ = [("n", C.c_int), ("u_stereo", c_float_p), ("v_stereo", c_float_p), ("idepth_min", c_float_p),
                ("idepth_min_stereo", c_float_p), ("idepth_max_stereo", c_float_p), ("idepth_stereo", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("gradH", c_float_p), ("energyTH", c_float_p),
                ("quality", c_float_p), ("lastTraceStatus", c_u8_p), ("lastTraceUV", c_float_p),
                ("lastTracePixelInterval", c_float_p)]


class TraceGeom(C.Structure):
    _c_name_ = "sdso_trace_geom_t"
    _fields_ = [("KRKi", C.c_float * 9), ("Kt", C.c_float * 3), ("aff", C.c_float * 2)]


class ImmGeom(C.Structure):
    """The geometry of one host keyframe into the newest frame (FullSystem.cpp:654-665)."""
    _c_name_ = "sdso_imm_geom_t"
    _fields_ = [("host_id", C.c_int), ("KRKi", C.c_float * 9), ("Kt", C.c_float * 3), ("aff", C.c_float * 2), ("KRi", C.c_float * 9), ("t", C.c_float * 3)]


INIT_NCOUNTS = 8   # non-zero map entries, numPoints[0], the histogram of the returned ImmaturePointStatus 0..5 over the Pnts


class InitPnts(C.Structure):
    """The Pnt members of CoarseInitializer::points[0] (CoarseInitializer.cpp:905-969)."""
    _c_name_ = "sdso_init_pnts_t"
    _fields_ = [("n", C.c_int), ("u", c_float_p), ("v", c_float_p), ("idepth", c_float_p), ("iR", c_float_p), ("my_type", c_float_p), ("status", c_u8_p)]


class InitPoints(C.Structure):
    """firstFrame->pointHessians after initializeFromInitializer STEP 3 (FullSystem.cpp:1533-1573)."""
    _c_name_ = "sdso_init_points_t"
    _fields_ = [("n", C.c_int), ("pnt", c_int_p), ("u", c_float_p), ("v", c_float_p), ("my_type", c_float_p), ("idepth", c_float_p), ("idepth_min", c_float_p),
                ("idepth_max", c_float_p), ("energyTH", c_float_p), ("color", c_float_p), ("weights", c_float_p)]


IMM_MAX_HOSTS = 8
IMM_NCOUNTS = 10   # lastTraceStatus histogram [0..5], forward GOOD, stereo outliers, intervals updated, unreadable
IMM_MATCH_NCOUNTS = 8   # walked, forward GOOD, back traces run, back GOOD, accepted, |du| >= 1, depth outside (0, max_depth), unreadable


class ImmMatchOut(C.Structure):
    """The per-point results of sdso_imm_stereo_match and its dense map (FullSystem.cpp:598-611)."""
    _c_name_ = "sdso_imm_match_out_t"
    _fields_ = [("accepted", c_u8_p), ("idepth", c_float_p), ("status_fwd", c_u8_p), ("status_back", c_u8_p), ("map", c_float_p)]


IMM_ACT_NCOUNTS = 17   # candidates, KEEP / DELETE / SELECT, toOptimize.size(), statuses -1 / 0 / 1, removed, the new count of every frame's group


class ImmActivate(C.Structure):
    """activatePointsMT STEP 2-5 on the resident set (FullSystem.cpp:837-957)."""
    _c_name_ = "sdso_imm_activate_t"
    _fields_ = [("nf", C.c_int), ("host_id", c_int_p), ("frame_slot", c_int_p), ("host_flagged", c_u8_p), ("geom", C.c_void_p),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_aff", c_float_p), ("w", C.c_int), ("h", C.c_int), ("K", C.c_float * 4),
                ("minObs", C.c_int), ("currentMinActDist", C.c_float), ("minTraceQuality", C.c_float)]


class ImmActivated(C.Structure):
    """One entry per selected candidate, in toOptimize order."""
    _c_name_ = "sdso_imm_activated_t"
    _fields_ = [("n", C.c_int), ("nf", C.c_int), ("frame", c_int_p), ("index", c_int_p), ("status", c_i8_p), ("idepth", c_float_p),
                ("res_state", c_u8_p), ("u", c_float_p), ("v", c_float_p), ("my_type", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("energyTH", c_float_p), ("color", c_float_p), ("weights", c_float_p), ("lastTraceStatus", c_u8_p)]


class Activate(C.Structure):
    _c_name_ = "sdso_activate_t"
    _fields_ = [("nf", C.c_int), ("w", C.c_int), ("h", C.c_int), ("n", C.c_int), ("minObs", C.c_int), ("K", C.c_float * 4),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_aff", c_float_p), ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("host", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("color", c_float_p), ("weights", c_float_p), ("energyTH", c_float_p)]


class DistMapGeom(C.Structure):
    """K[1] * R * Ki[0] and K[1] * t of one keyframe into the newest (CoarseTracker.cpp:1235-1236)."""
    _c_name_ = "sdso_distmap_geom_t"
    _fields_ = [("KRKi", C.c_float * 9), ("Kt", C.c_float * 3)]


class ActivateSelect(C.Structure):
    """The candidates of FullSystem::activatePointsMT STEP 2 (FullSystem.cpp:837-902)."""
    _c_name_ = "sdso_activate_select_t"
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("ngeom", C.c_int), ("geom", C.POINTER(DistMapGeom)), ("host_flagged", c_u8_p),
                ("n", C.c_int), ("point_geom", c_int_p), ("u", c_float_p), ("v", c_float_p), ("idepth_min", c_float_p), ("idepth_max", c_float_p),
                ("quality", c_float_p), ("lastTracePixelInterval", c_float_p), ("lastTraceStatus", c_u8_p), ("my_type", c_float_p),
                ("currentMinActDist", C.c_float), ("minTraceQuality", C.c_float)]


class StereoMatch(C.Structure):
    _c_name_ = "sdso_stereo_match_t"
    _fields_ = [("n", C.c_int), ("u", c_float_p), ("v", c_float_p), ("idepth_min_stereo", c_float_p), ("idepth_max_stereo", c_float_p),
                ("back_idepth_min_stereo", c_float_p), ("back_idepth_max_stereo", c_float_p), ("status_fwd", c_u8_p), ("status_back", c_u8_p),
                ("idepth_stereo", c_float_p), ("idepth_min_out", c_float_p), ("idepth_max_out", c_float_p), ("fwd_uv", c_float_p),
                ("back_uv", c_float_p)]


class G2oTrackEval(C.Structure):
    """One EdgeSE3PosePhotoDSO evaluation point (fork-live tracker, dso_g2o_edge.cpp:395-500)."""
    _c_name_ = "sdso_g2o_track_eval_t"
    _fields_ = [("lvl", C.c_int), ("w", C.c_int), ("h", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Ki", C.c_float * 9), ("RKi", C.c_float * 9), ("t_cull", C.c_float * 3),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("ab", C.c_float * 2), ("b0", C.c_double), ("cutoffTH", C.c_float), ("huberTH", C.c_float)]


class G2oLba(C.Structure):
    """EdgeLBASE3PosePhotoIdepthCamDSO batch (dso_g2o_edge.cpp:5-282)."""
    _c_name_ = "sdso_g2o_lba_t"
    _fields_ = [("nf", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("frame_slot", c_int_p), ("dI", C.POINTER(c_float_p)),
                ("pair_R", c_float_p), ("pair_t", c_float_p), ("pair_ab", c_float_p), ("host_b0", c_double_p),
                ("frameEnergyTH", c_float_p), ("cam", C.c_double * 4), ("host", c_int_p), ("target", c_int_p),
                ("u", c_float_p), ("v", c_float_p), ("idepth", c_double_p), ("color", c_float_p), ("weights", c_float_p)]


class G2oLbaWindow(C.Structure):
    """The window graph of FullSystem::optimize, fork-live (FullSystemOptimize.cpp:455-542)."""
    _c_name_ = "sdso_g2o_lba_window_t"
    _fields_ = [("nf", C.c_int), ("nr", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("frame_slot", c_int_p), ("Ttw", C.POINTER(SE3)), ("target_aff", C.POINTER(Aff)), ("ab_exposure", c_float_p),
                ("host_b0", c_double_p), ("frameEnergyTH", c_float_p), ("host", c_int_p), ("target", c_int_p),
                ("u", c_float_p), ("v", c_float_p), ("color", c_float_p), ("weights", c_float_p)]


class G2oLbaState(C.Structure):
    """The vertex estimates, in and out."""
    _c_name_ = "sdso_g2o_lba_state_t"
    _fields_ = [("Twh", C.POINTER(SE3)), ("host_aff", C.POINTER(Aff)), ("cam", C.c_double * 4), ("idepth", c_double_p)]


class G2oLbaOpt(C.Structure):
    _c_name_ = "sdso_g2o_lba_opt_t"
    _fields_ = [("max_iterations", C.c_int), ("lambda_init", C.c_double), ("gain_threshold", C.c_double), ("max_trials", C.c_int)]


G2O_LBA_MAX_RECORDED = 64


class G2oLbaResult(C.Structure):
    _c_name_ = "sdso_g2o_lba_result_t"
    _fields_ = [("iterations", C.c_int), ("stop", C.c_int), ("n_active", C.c_int),
                ("trials", C.c_int * G2O_LBA_MAX_RECORDED), ("lambda_", C.c_double * G2O_LBA_MAX_RECORDED), ("chi2", C.c_double * G2O_LBA_MAX_RECORDED),
                ("chi2_final", C.c_double), ("rmse", C.c_float),
                ("state", c_u8_p), ("energy", c_float_p), ("centerProjectedTo", c_float_p), ("edge_level", c_u8_p),
                ("idepth_hessian", c_float_p), ("active", c_u8_p)]


class PoolStats(C.Structure):
    """The counters of a device buffer pool."""
    _c_name_ = "sdso_pool_stats_t"
    _fields_ = [(k, C.c_longlong) for k in ("hits", "misses", "frees", "host_waits", "overflow_waits", "parked_buffers", "parked_bytes")]


STRUCTS = [v for v in list(globals().values()) if isinstance(v, type) and issubclass(v, C.Structure) and hasattr(v, "_c_name_")]
