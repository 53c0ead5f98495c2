"""The signatures of libsdso_hip.so and its loader.  SIGNATURES names every function include/sdso_abi.h declares once, in the header's
sections; it is the export list (EXPORTED_SYMBOLS), and tests/test_abi_layout_cpu.py holds it to the header's prototypes.

There is no CPU fallback: load() raises if the HIP library has not been built."""
import ctypes as C
import os
from ctypes import POINTER as P, c_char_p, c_long, c_ulonglong, c_int as I, c_float as F, c_double as D, c_size_t as Z, c_void_p as vp

from .abi_types import *   # noqa: F401,F403  (the structure classes the table names)
from .abi_types import c_float_p as fP, c_double_p as dP, c_int_p as iP, c_u8_p as bP

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDSO_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libsdso_hip.so")   # override: A/B experiments only

# name -> argument types, or (argument types, return type) where the function does not return int
SIGNATURES = {
    # context
    "sdso_ctx_create": [I, P(vp)],
    "sdso_ctx_destroy": ([vp], None),
    "sdso_last_error": ([vp], c_char_p),
    "sdso_ctx_stream": ([vp], vp),
    "sdso_ctx_sync": [vp],
    "sdso_ctx_partition_cus": [vp, I, I],
    "sdso_prof_enable": [vp, I],
    "sdso_prof_reset": [vp],
    "sdso_prof_read": [vp, c_char_p, dP, P(c_long)],
    "sdso_selftest_se3": [vp, I, dP, dP, dP, dP],
    # pyramids
    "sdso_pyramid_levels": [I, I],
    "sdso_upload_pyramid": [vp, I, I, iP, iP, P(fP)],
    "sdso_make_pyramid": [vp, I, I, I, fP],
    "sdso_set_gamma": [vp, fP],
    "sdso_gamma_from_binv": [fP, fP],
    "sdso_download_pyramid_level": [vp, I, I, fP],
    "sdso_download_abs_grad": [vp, I, I, fP],
    "sdso_release_pyramid": [vp, I],
    # frame ingest
    "sdso_undistort_make_remap": [I, dP, I, I, I, I, I, fP, dP, fP, fP, iP],
    "sdso_ingest_calib_create": [vp, I, I, I, I, I, fP, fP, I, fP, fP, I, I],
    "sdso_ingest_calib_release": [vp, I],
    "sdso_ingest_frame": [vp, I, I, iP, P(vp), fP, F, fP],
    # coarse tracker
    "sdso_track_set_ref": [vp, I, I, I, fP, fP, fP, fP],
    "sdso_track_release_ref": [vp, I],
    "sdso_track_make_ref": [vp, I, I, I, iP, iP, fP, fP, iP],
    "sdso_track_make_ref_from_window": [vp, I, I, I, F, iP, I, iP, iP, iP],
    "sdso_track_get_ref_points": [vp, I, iP, iP, iP, iP, fP, bP, bP, fP, fP],
    "sdso_track_get_ref": [vp, I, I, iP, fP, fP, fP, fP],
    "sdso_track_keep_depth_map": [vp, I],
    "sdso_track_depth_image": [vp, I, I, fP, fP, bP, fP, iP],
    "sdso_track_depth_image_dev": [vp, I, P(vp), P(vp), iP, iP],
    "sdso_track_calc_res_gs": [vp, I, I, P(TrackEval), dP, dP, dP, iP, bP],
    "sdso_track_calc_res_gs_batch": [vp, I, iP, iP, P(TrackEval), dP, dP, dP, iP],
    "sdso_track_batch_prepare": [vp, I, iP, iP, P(TrackEval)],
    "sdso_track_batch_enqueue": [vp],
    "sdso_track_batch_fetch": [vp, dP, dP, dP, iP],
    "sdso_track_make_eval": ([P(TrackParams), I, P(SE3), P(Aff), F, P(TrackEval)], None),
    "sdso_track_newest_coarse": [vp, I, I, P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "sdso_track_newest_coarse_batch": [vp, I, iP, iP, P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "sdso_track_tries_replay": [I, P(SE3), P(Aff), P(TrackTry), dP, D, P(TrackTriesResult)],
    "sdso_track_new_coarse": [vp, I, I, P(TrackParams), I, P(SE3), P(Aff), dP, D, P(TrackTriesResult), P(TrackTry)],
    # hand-off between contexts
    "sdso_pyramid_export": [vp, I, P(vp)],
    "sdso_pyramid_import": [vp, I, vp],
    "sdso_track_export_ref": [vp, I, P(vp)],
    "sdso_track_import_ref": [vp, I, vp],
    "sdso_shared_info": [vp, iP, iP, iP],
    "sdso_shared_release": ([vp], None),
    "sdso_shared_debug_buffers": [vp, I, I, P(c_ulonglong), iP],
    # device buffer pool
    "sdso_pool_create": [I, Z, P(vp)],
    "sdso_ctx_set_pool": [vp, vp],
    "sdso_pool_stats": [vp, P(PoolStats)],
    "sdso_pool_trim": [vp, Z],
    "sdso_pool_release": ([vp], None),
    # windowed bundle adjustment
    "sdso_ba_upload_window": [vp, I, P(BAWindow)],
    "sdso_ba_release_window": [vp, I],
    "sdso_ba_linearize": [vp, I, dP],
    "sdso_ba_get_linearization": [vp, I, fP, bP, fP, fP, fP, fP],
    "sdso_ba_apply_res": [vp, I],
    "sdso_ba_get_residual_state": [vp, I, bP, bP, fP],
    "sdso_ba_get_ef_jacobians": [vp, I, fP],
    "sdso_ba_accumulate": [vp, I],
    "sdso_ba_accum_floats": [I],
    "sdso_ba_accum_dev": [vp, I, P(vp)],
    "sdso_ba_get_accumulators": [vp, I, fP],
    "sdso_ba_set_accumulators": [vp, I, fP],
    "sdso_ba_get_point_terms": [vp, I, fP, fP, fP, fP, fP],
    "sdso_ba_solve": [vp, I, I, D, dP, dP, dP, dP, dP],
    "sdso_ba_resubstitute": [vp, I, dP, dP, dP],
    "sdso_ba_get_point_steps": [vp, I, fP],
    "sdso_ba_optimize": [vp, I, I, dP, fP, bP, P(BAOptResult)],
    "sdso_ba_get_post_state": [vp, I, P(BAPostState)],
    "sdso_ba_get_counts": [vp, I, iP, iP, iP],
    "sdso_ba_flag_points": [vp, I, P(BAFlagPoints), bP, iP, iP],
    "sdso_ba_marginalize_points": [vp, I, bP, dP, dP],
    "sdso_ba_marginalize_frame": [I, I, dP, dP, dP, dP, dP, dP],
    "sdso_ba_calc_energies": [vp, I, dP, dP],
    "sdso_ba_get_deltas": [vp, I, fP, dP, dP, fP],
    "sdso_ba_get_tables": [vp, I, fP, dP, dP, fP],
    "sdso_ba_get_state": [vp, I, dP, fP, bP],
    "sdso_ba_marginalize_frame_dev": [vp, I, I, dP, dP],
    "sdso_ba_adopt_prior": [vp, I, I],
    "sdso_ba_window_plan": [I, I, I, iP, iP, iP, P(BAWindowEdit), iP, iP, iP, iP, iP, iP],
    "sdso_ba_window_update": [vp, I, P(BAWindowEdit)],
    "sdso_ba_window_update_activated": [vp, I, P(BAWindowEdit), iP, iP, iP, iP],
    "sdso_ba_window_get_order": [vp, I, iP, iP, iP],
    "sdso_ba_keep_projections": [vp, I, I],
    "sdso_ba_batch_create": [vp, I, iP],
    "sdso_ba_batch_accumulate": [vp],
    "sdso_ba_batch_linearize": [vp],
    "sdso_ba_batch_schur": [vp],
    "sdso_ba_batch_set_materialize": [vp, I],
    "sdso_ba_batch_keep_system": [vp, I],
    "sdso_ba_batch_exchange_mode": [vp, I],
    "sdso_ba_batch_solve": [vp, D, I],
    "sdso_ba_batch_accum_dev": [vp, P(vp), P(c_long)],
    "sdso_ba_batch_get_x": [vp, dP],
    "sdso_ba_get_stitched": [vp, I] + [dP] * 6,
    "sdso_ba_batch_optimize": [vp, I, P(BAOptResult)],
    "sdso_ba_batch_optimize_begin": [vp, I],
    "sdso_ba_batch_step": [vp],
    "sdso_ba_batch_solve_step": [vp, D, I],
    "sdso_ba_batch_optimize_end": [vp, P(BAOptResult)],
    # multi-GPU exchange
    "sdso_comm_unique_id": [vp],
    "sdso_comm_init": [vp, I, I, vp],
    "sdso_comm_attach": [vp, vp],
    "sdso_comm_init_host": [vp, I, I, HOST_ALLREDUCE_FN, HOST_ALLGATHER_FN, vp],
    "sdso_comm_info": [vp, iP, iP],
    "sdso_comm_destroy": [vp],
    "sdso_ba_allreduce": [vp],
    "sdso_ba_allreduce_window": [vp, I],
    # static stereo
    "sdso_immature_init_batch": [vp, I, I, fP, fP, fP, fP, fP, fP],
    "sdso_trace_stereo_batch": [vp, I, fP, F, I, P(TracePoints), bP],
    "sdso_trace_stereo_prepare": [vp, I, fP, F, I, P(TracePoints)],
    "sdso_trace_stereo_enqueue": [vp],
    "sdso_trace_stereo_fetch": [vp, P(TracePoints), bP],
    "sdso_pixel_select": [vp, I, F, I, F, iP, fP, iP],
    "sdso_pixel_selector_pattern": [I, bP],
    "sdso_trace_on_batch": [vp, I, I, P(TraceGeom), iP, P(TracePoints), bP],
    "sdso_activate_points_batch": [vp, P(Activate), c_i8_p, fP, bP],
    "sdso_distmap_make": [vp, I, I, I, P(DistMapGeom), I, iP, fP, fP, fP, iP],
    "sdso_distmap_make_from_window": [vp, I, I, I, P(DistMapGeom), bP, iP],
    "sdso_distmap_add": [vp, I, iP, iP],
    "sdso_distmap_get": [vp, fP],
    "sdso_activate_select": [vp, P(ActivateSelect), bP, iP, iP, iP],
    "sdso_stereo_match_batch": [vp, I, I, fP, F, I, P(StereoMatch)],
    # the stereo initialiser
    "sdso_init_set_first_stereo": [vp, I, I, fP, F, fP, iP, iP],
    "sdso_init_get_pnts": [vp, P(InitPnts)],
    "sdso_init_from_initializer": [vp, bP, iP, iP],
    "sdso_init_get_points": [vp, P(InitPoints)],
    "sdso_init_release": [vp],
    # the device-resident immature points
    "sdso_imm_add_frame": [vp, I, I, fP, iP],
    "sdso_imm_trace": [vp, I, I, I, P(ImmGeom), fP, fP, F, iP],
    "sdso_imm_stereo_match": [vp, I, I, I, fP, F, F, I, P(ImmMatchOut), iP],
    "sdso_imm_stereo_match_fetch": [vp, P(ImmMatchOut), iP],
    "sdso_imm_stereo_map_dev": [vp, P(vp), iP, iP],
    "sdso_imm_count": [vp, I, iP],
    "sdso_imm_get": [vp, I, P(TracePoints), fP],
    "sdso_imm_remove_order": [I, bP, iP, iP],
    "sdso_imm_remove": [vp, I, I, bP],
    "sdso_imm_release_host": [vp, I],
    "sdso_imm_put_host": [vp, I, I, I, P(TracePoints), fP],
    "sdso_imm_activate": [vp, P(ImmActivate), iP],
    "sdso_imm_activate_fetch": [vp, P(ImmActivated), bP],
    # the fork's live g2o factors
    "sdso_trace_set_gn_mode": [vp, I],
    "sdso_g2o_track_add_edges": [vp, I, I, P(G2oTrackEval), dP, iP, bP, fP],
    "sdso_g2o_track_linearize": [vp, I, I, P(G2oTrackEval), dP, dP, dP, dP, dP],
    "sdso_g2o_track_newest_coarse": [vp, I, I, P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "sdso_g2o_track_newest_coarse_batch": [vp, I, iP, iP, P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "sdso_g2o_track_new_coarse": [vp, I, I, P(TrackParams), I, P(SE3), P(Aff), dP, D, P(TrackTriesResult), P(TrackTry)],
    "sdso_g2o_lba_eval": [vp, P(G2oLba), dP, dP, bP, fP, fP, fP, bP],
    "sdso_g2o_lba_optimize": [vp, P(G2oLbaWindow), P(G2oLbaOpt), P(G2oLbaState), P(G2oLbaResult)],
    "sdso_g2o_lba_optimize_enqueue": [vp, P(G2oLbaWindow), P(G2oLbaOpt), P(G2oLbaState)],
    "sdso_g2o_lba_optimize_done": [vp],
    "sdso_g2o_lba_optimize_fetch": [vp, P(G2oLbaState), P(G2oLbaResult)],
    "sdso_g2o_lba_optimize_resident": [vp, P(G2oLbaWindow), P(G2oLbaOpt), P(G2oLbaState), P(G2oLbaResult)],
    # the device-resident map
    "sdso_map_update": [vp, I, P(MapUpdate)],
    "sdso_map_counts": [vp, I, iP],
    "sdso_map_get": [vp, I, I, fP],
    "sdso_map_put": [vp, I, I, I, fP],
    "sdso_map_release_keyframe": [vp, I],
    "sdso_map_clear": [vp],
    "sdso_map_cloud": [vp, P(MapCloud), fP, bP, iP, iP],
    "sdso_map_cloud_dev": [vp, P(vp), P(vp), iP],
}
EXPORTED_SYMBOLS = list(SIGNATURES)


def declare(L, signatures):
    """Set argtypes and restype of every function of the table on the loaded library L."""
    for name, sig in signatures.items():
        f = getattr(L, name)
        f.argtypes, f.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
    return L


_lib = None


def load():
    """Load libsdso_hip.so (built by `make -C stereo-dso-g2o_amd/csrc` or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libsdso_hip.so is not built (%s): run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
        _lib = declare(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib
