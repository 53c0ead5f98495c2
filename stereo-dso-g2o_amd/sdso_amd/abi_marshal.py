"""numpy arrays into the structures of abi_types: the one dtype -> pointer rule (ptr), the one way a structure's pointer members are
set (bind: through ptr, and the structure keeps the arrays alive), and the builders of the larger structures."""
import ctypes as C

import numpy as np

from .abi_types import (c_float_p, c_double_p, c_int_p, c_u8_p, c_i8_p, BAWindow, BAWindowEdit, BAPostState, BAFlagPoints, TracePoints,
                        DistMapGeom)

POINTER_OF = {np.dtype(np.float32): c_float_p, np.dtype(np.float64): c_double_p, np.dtype(np.int32): c_int_p, np.dtype(np.uint8): c_u8_p,
              np.dtype(np.int8): c_i8_p}
_DTYPE_OF = {t: d for d, t in POINTER_OF.items()}


def ptr(a):
    """The pointer of a's own element type to a's data.  TypeError for any other dtype and for an array that is not C-contiguous."""
    t = POINTER_OF.get(getattr(a, "dtype", None))
    if t is None:
        raise TypeError("ptr: a float32 / float64 / int32 / uint8 / int8 array is needed, not %r" % (getattr(a, "dtype", type(a)),))
    if not a.flags.c_contiguous:
        raise TypeError("ptr: the array is not C-contiguous")
    return a.ctypes.data_as(t)


def bind(S, arrays):
    """Set member k of the structure S to ptr(a) for every (k, a) of the dict `arrays` (a = None: a null pointer).  ctypes refuses a
    pointer of another element type than the member's, so a wrong dtype is a TypeError; a name that is no member is an AttributeError.
    S keeps the arrays alive.  Returns S."""
    held = S.__dict__.setdefault("_bound", {})
    for k, a in arrays.items():
        getattr(type(S), k)
        setattr(S, k, None if a is None else ptr(a))
        held[k] = a
    return S


def as_members(S, values):
    """dict of array-likes -> dict of C-contiguous arrays in the element type of S's member of the same name; None entries are left out.
    The builders' conversion: bind itself converts nothing."""
    types = dict(S._fields_)
    return {k: np.ascontiguousarray(v, _DTYPE_OF[types[k]]) for k, v in values.items() if v is not None}


# unchecked one-liners for call arguments in timed loops; everything that fills a structure goes through bind
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
    return bind(BAPostState(), d), d


def make_flag_points(frame_marg, last_gone=None, minGoodActiveResForMarg=3, minGoodResForMarg=4, minIdepthH_marg=50.0):
    """Fill a BAFlagPoints.  frame_marg: nf flags; last_gone: np*2 bytes (0/1/2 or 255) or None.  Returns (struct, keep-alive list)."""
    F = BAFlagPoints()
    d = as_members(F, dict(frame_marg=frame_marg, last_gone=None if last_gone is None else np.asarray(last_gone).reshape(-1)))
    bind(F, d)
    F.minGoodActiveResForMarg, F.minGoodResForMarg, F.minIdepthH_marg = int(minGoodActiveResForMarg), int(minGoodResForMarg), float(minIdepthH_marg)
    return F, list(d.values())


def make_distmap_geoms(KRKi, Kt):
    """(ng, 3, 3) and (ng, 3) float32 arrays -> a ctypes array of DistMapGeom."""
    KRKi = np.ascontiguousarray(KRKi, np.float32).reshape(-1, 9)
    Kt = np.ascontiguousarray(Kt, np.float32).reshape(-1, 3)
    G = (DistMapGeom * max(1, len(KRKi)))()
    for g in range(len(KRKi)):
        G[g].KRKi[:] = KRKi[g].tolist()
        G[g].Kt[:] = Kt[g].tolist()
    return G


_WINDOW_ARRAYS = ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID", "u", "v", "idepth", "idepth_zero", "color", "weights",
                  "host", "hasDepthPrior", "res_point", "res_target", "res_state", "HM", "bM")
_WINDOW_OPTIONAL = ("maxRelBaseline", "numGoodResiduals", "res_isNew")


def make_ba_window(win, frame_slots=None, dI_list=None):
    """Fill a BAWindow from the dict synth.ba_window() returns.  Keeps references alive in `keep`."""
    W = BAWindow()
    W.nf, W.np, W.nr, W.w, W.h = win["nf"], win["np"], win["nr"], win["w"], win["h"]
    W.calib_value_scaled[:] = list(win["calib_value_scaled"])
    W.calib_value_zero[:] = list(win["calib_value_zero"])
    d = {k: win[k] for k in _WINDOW_ARRAYS}
    d.update({k: win.get(k) for k in _WINDOW_OPTIONAL}, frame_slot=frame_slots)
    d = as_members(W, d)
    bind(W, d)
    keep = list(d.values())
    if dI_list is not None:
        imgs = [np.ascontiguousarray(a, np.float32) for a in dI_list]
        ptrs = (c_float_p * len(imgs))(*[ptr(a) for a in imgs])
        keep += imgs + [ptrs]
        W.dI = C.cast(ptrs, C.POINTER(c_float_p))
    W.solverMode, W.forceAcceptStep = int(win["solverMode"]), int(win["forceAcceptStep"])
    W.affineOptModeA, W.affineOptModeB = float(win["affineOptModeA"]), float(win["affineOptModeB"])
    return W, keep


def make_window_edit(drop_res=None, remove_points=None, drop_point=None, remove_frames=None, add_frames=None, add_res=None, add_points=None):
    """Fill a BAWindowEdit.  drop_res / remove_points / remove_frames: index sequences (their order is the order of the drops);
    drop_point: np flags; add_frames: dict(evalPT (k,12), state (k,10), state_zero (k,10), ab_exposure, frameEnergyTH, frameID,
    frame_slot); add_res: dict(point, target, state[, isNew]); add_points: dict(host, u, v, idepth, idepth_zero, color (k,8),
    weights (k,8), hasDepthPrior[, maxRelBaseline, numGoodResiduals], res_point, res_target, res_state[, res_isNew]).  Every index is in
    the numbering of the window before the call.  Returns (struct, keep-alive list)."""
    E = BAWindowEdit()
    v = dict(drop_res=drop_res, remove_points=remove_points, drop_point=drop_point, remove_frames=remove_frames)
    if add_frames is not None:
        v.update({k: add_frames[k] for k in ("frameID", "evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frame_slot")})
    if add_res is not None:
        v.update({"add_res_" + k: add_res[k] for k in ("point", "target", "state")}, add_res_isNew=add_res.get("isNew"))
    if add_points is not None:
        v.update({"pt_" + k: add_points[k] for k in ("host", "u", "v", "idepth", "idepth_zero", "color", "weights", "hasDepthPrior",
                                                     "res_point", "res_target", "res_state")})
        v.update({"pt_" + k: add_points.get(k) for k in ("maxRelBaseline", "numGoodResiduals", "res_isNew")})
    d = as_members(E, v)
    bind(E, d)
    for count, member in (("n_drop_res", "drop_res"), ("n_remove_points", "remove_points"), ("n_remove_frames", "remove_frames"),
                          ("n_add_frames", "frameID"), ("n_add_res", "add_res_point"), ("n_add_points", "pt_host"), ("n_pt_res", "pt_res_point")):
        if member in d:
            setattr(E, count, len(d[member]))
    return E, list(d.values())


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
    P = bind(TracePoints(), d)
    P.n = n
    return P, d
