"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes loader for oracle/liboracle.so (strict-IEEE CPU restatement, the parity checker) and
oracle/liboracle_fast.so (same sources, -O3 -march=native: bench.py's cpu_baseline "port").
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "stereo-dso-g2o_amd"))
from sdso_amd.abi import (G2oTrackEval, G2oLba, Activate, TraceGeom, TrackEval, SE3, Aff, TrackParams, TrackResult, BAWindow, BAOptResult, BAPostState, TracePoints,  # noqa: E402
                          c_float_p, c_double_p, c_int_p, c_u8_p, c_i8_p, declare)

_libs = {}
P, I, F, D, vp = C.POINTER, C.c_int, C.c_float, C.c_double, C.c_void_p
fP, dP, iP, bP = c_float_p, c_double_p, c_int_p, c_u8_p
# name -> argument types, or (argument types, return type) where the function does not return int; applied by sdso_amd.abi.declare
SIGNATURES = {
    "orc_se3_exp": ([dP, P(SE3)], None),
    "orc_se3_log": ([P(SE3), dP], None),
    "orc_se3_adj": ([P(SE3), dP], None),
    "orc_se3_mul": ([P(SE3), P(SE3), P(SE3)], None),
    "orc_se3_inv": ([P(SE3), P(SE3)], None),
    "orc_mat3f_inv": ([fP, fP], None),
    "orc_ldlt_solve": [I, dP, dP, dP],
    "orc_pyramid_levels": [I, I],
    "orc_make_images": ([fP, I, I, I, P(fP)], None),
    "orc_track_calc_res_gs": [I, fP, fP, fP, fP, fP, P(TrackEval), dP, dP, dP, iP, bP, fP, I],
    "orc_track_make_eval": ([P(TrackParams), I, P(SE3), P(Aff), F, P(TrackEval)], None),
    "orc_track_newest_coarse": [iP, P(fP), P(fP), P(fP), P(fP), P(fP), P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "orc_make_coarse_depth": [I, iP, iP, P(fP), I, iP, iP, fP, fP, iP, P(fP), P(fP), P(fP), P(fP)],
    "orc_ba_get_stitched": [vp] + [dP] * 6,
    "orc_track_last_margins": ([dP], None),
    "orc_ba_create": ([P(BAWindow)], vp),
    "orc_ba_destroy": ([vp], None),
    "orc_ba_set_threads": [vp, I],
    "orc_ba_linearize": [vp, dP],
    "orc_ba_get_linearization": [vp, fP, bP, fP, fP, fP, fP],
    "orc_ba_apply_res": [vp],
    "orc_ba_get_ef_jacobians": [vp, fP],
    "orc_ba_get_residual_state": [vp, bP, bP, fP],
    "orc_ba_accumulate": [vp],
    "orc_ba_accum_floats": [I],
    "orc_ba_get_accumulators": [vp, fP],
    "orc_set_acc64": ([I], None),
    "orc_ba_get_accumulators_f64": [vp, dP],
    "orc_ba_get_point_terms": [vp, fP, fP, fP, fP, fP],
    "orc_ba_solve": [vp, I, D, dP, dP, dP, dP, dP],
    "orc_ba_get_point_steps": [vp, fP],
    "orc_ba_optimize": [vp, I, dP, fP, bP, P(BAOptResult)],
    "orc_ba_marginalize_points": [vp, bP, dP, dP],
    "orc_ba_get_post_state": [vp, P(BAPostState)],
    "orc_ba_get_x_trace": [vp, dP, I],
    "orc_ba_get_step_trace": [vp, fP, I],
    "orc_ba_calc_energies": [vp, dP, dP],
    "orc_ba_get_deltas": [vp, fP, dP, dP, fP],
    "orc_ba_get_tables": [vp, fP, dP, dP, fP],
    "orc_immature_init_batch": [fP, I, I, I, fP, fP, fP, fP, fP, fP],
    "orc_pixel_select": [P(fP), I, I, F, I, F, iP, fP],
    "orc_set_gamma": ([fP], None),
    "orc_gamma_from_binv": ([fP, fP], None),
    "orc_selector_random_pattern": ([I, bP], None),
    "orc_marginalize_frame": [I, I, dP, dP, dP, dP, dP, dP],
    "orc_activate_points": [P(Activate), c_i8_p, fP, bP],
    "orc_trace_on_batch": [fP, I, I, I, P(TraceGeom), iP, P(TracePoints), bP],
    "orc_trace_stereo_batch": [fP, I, I, fP, F, I, P(TracePoints), bP],
    "orc_trace_stereo_batch_gn": [fP, I, I, fP, F, I, P(TracePoints), bP, I],
    "orc_g2o_track_add_edges": [I, fP, fP, fP, fP, fP, P(G2oTrackEval), dP, bP, fP],
    "orc_g2o_track_linearize": [I, bP, fP, fP, fP, P(G2oTrackEval), dP, dP, dP, dP, dP],
    "orc_g2o_track_newest_coarse": [iP, P(fP), P(fP), P(fP), P(fP), P(fP), P(TrackParams), P(SE3), P(Aff), P(TrackResult)],
    "orc_g2o_lba_eval": [P(G2oLba), dP, dP, bP, fP, fP, fP, bP],
}


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


FAST_FLAGS_SHIPPED = "-O3 -march=x86-64-v3 -mtune=generic"   # oracle/Makefile FAST_FLAGS


def build_native(out_dir="/tmp"):
    """The timed CPU baseline rebuilt ON THE HOST THAT TIMES IT (-O3 -march=native, the reference's own flags, CMakeLists.txt:83-84).
    Returns (path, flags), or (None, reason) when no compiler is there."""
    import shutil
    if not shutil.which(os.environ.get("CXX", "g++")):
        return None, "no g++ on the timed host"
    out = os.path.join(out_dir, "liboracle_native_%d.so" % os.getpid())
    flags = "-O3 -march=native"
    try:
        subprocess.check_call(["make", "-s", "-C", _HERE, "native", "FAST_FLAGS=" + flags, "FAST_OUT=" + out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    except (subprocess.SubprocessError, OSError) as e:
        return None, "native build failed: %r" % (e,)
    return out, flags


def load(fast=False, path=None):
    name = path or ("liboracle_fast.so" if fast else "liboracle.so")
    if name in _libs:
        return _libs[name]
    path = path or os.path.join(_HERE, name)
    if not os.path.exists(path):
        build()
    L = _libs[name] = declare(C.CDLL(path), SIGNATURES)
    return L


def make_coarse_depth(L, u, v, new_idepth, weight, ref_pyr):
    """orc_make_coarse_depth on numpy arrays: a list (per level) of dicts u, v, idepth, color (float32), like the tracker template."""
    import numpy as np
    levels = len(ref_pyr)
    ws = (C.c_int * levels)(*[p.shape[1] for p in ref_pyr]); hs = (C.c_int * levels)(*[p.shape[0] for p in ref_pyr])
    imgs = [np.ascontiguousarray(p, np.float32) for p in ref_pyr]
    dI = (c_float_p * levels)(*[a.ctypes.data_as(c_float_p) for a in imgs])
    out = [[np.zeros(p.shape[0] * p.shape[1], np.float32) for p in ref_pyr] for _ in range(4)]
    ptrs = [(c_float_p * levels)(*[a.ctypes.data_as(c_float_p) for a in arrs]) for arrs in out]
    pc_n = (C.c_int * levels)()
    ui, vi = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32)
    idp, wgt = np.ascontiguousarray(new_idepth, np.float32), np.ascontiguousarray(weight, np.float32)
    L.orc_make_coarse_depth(levels, ws, hs, dI, len(ui), ui.ctypes.data_as(c_int_p), vi.ctypes.data_as(c_int_p), idp.ctypes.data_as(c_float_p),
                            wgt.ctypes.data_as(c_float_p), pc_n, *ptrs)
    return [dict(u=out[0][l][:pc_n[l]].copy(), v=out[1][l][:pc_n[l]].copy(), idepth=out[2][l][:pc_n[l]].copy(), color=out[3][l][:pc_n[l]].copy())
            for l in range(levels)]
