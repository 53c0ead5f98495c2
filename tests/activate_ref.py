"""CPU statement of sdso_imm_activate: FullSystem::activatePointsMT STEP 2-5 (FullSystem.cpp:837-957) on the immature points of a window,
composed from what the other statements already provide:

  STEP 2  distmap_ref.select on the flattened candidates (hosts in frame order, each group in its order), re-growing the map
  STEP 3  the oracle's orc_activate_points (optimizeImmaturePoint, FullSystemOptPoint.cpp:52-238) on the SELECTed candidates
  STEP 4  :919-945 — an entry leaves if STEP 2 deleted it, or it was selected and came back 1 or -1, or came back 0 with IPS_OOB
  STEP 5  immature_ref.remove (the swap-with-back loop, :948-957) per group

A window is a dict: groups (one dict of arrays per frame as immature_ref keeps them, or None for a frame without a group; the last
frame is the newest), imgs (level-0 {I, dx, dy} per frame), flagged, KRKi / Kt (nf-1), pair_R / pair_t / pair_aff (nf*nf), K4, w, h."""
import ctypes as C

import numpy as np

from sdso_amd import abi
import distmap_ref as D
import immature_ref as R

f32 = np.float32
COPIED = ("u", "v", "my_type", "idepth_min", "idepth_max", "energyTH", "color", "weights", "lastTraceStatus")   # HessianBlocks.cpp:35-70 + :937


def closed_form_order(flags):
    """The order of STEP 5 without the loop, as the device computes it: with m survivors, survivors at indices < m stay; the flagged
    indices < m, ascending, receive the survivors at indices >= m, descending."""
    flags = np.asarray(flags, bool)
    n = len(flags)
    m = n - int(flags.sum())
    src = np.arange(m)
    holes = np.nonzero(flags[:m])[0]
    back = np.nonzero(~flags[m:])[0][::-1] + m
    assert len(holes) == len(back)
    src[holes] = back
    return list(src)


def activate(orc, win, m, min_obs, min_act_dist, min_trace_quality=3.0):
    """Runs the call on win["groups"] (changed in place) and the flat map list `m` (re-grown in place).
    -> dict(counts, decision, row, records: dict of arrays in toOptimize order)"""
    groups, nf = win["groups"], len(win["groups"])
    w, h = win["w"], win["h"]
    walked = [g for g in range(nf - 1) if groups[g] is not None and len(groups[g]["u"])]
    cat = lambda k, dt=f32: (np.concatenate([groups[g][k] for g in walked]) if walked else np.zeros(0, dt))
    frame = np.concatenate([np.full(len(groups[g]["u"]), g, np.int32) for g in walked]) if walked else np.zeros(0, np.int32)
    index = np.concatenate([np.arange(len(groups[g]["u"]), dtype=np.int32) for g in walked]) if walked else np.zeros(0, np.int32)
    n = len(frame)
    # ---- STEP 2
    sel = D.select(m, w, h, win["KRKi"], win["Kt"], win["flagged"], frame, cat("u"), cat("v"), cat("idepth_min"), cat("idepth_max"), cat("quality"),
                   cat("lastTracePixelInterval"), cat("lastTraceStatus", np.uint8), cat("my_type"), min_act_dist, min_trace_quality)
    dec = sel["decision"]
    opt = np.nonzero(dec == D.SELECT)[0]
    ns = len(opt)
    # ---- STEP 3
    rec = dict(frame=frame[opt].copy(), index=index[opt].copy())
    for k in COPIED:
        rec[k] = np.ascontiguousarray(cat(k, np.uint8 if k == "lastTraceStatus" else f32)[opt]) if n else np.zeros((0, 8) if k in ("color", "weights") else 0,
                                                                                                                   np.uint8 if k == "lastTraceStatus" else f32)
    status, idepth, res_state = np.zeros(ns, np.int8), np.zeros(ns, f32), np.full((ns, nf), 255, np.uint8)
    if ns:
        A = abi.Activate()
        keep = [np.ascontiguousarray(win[k], f32) for k in ("pair_R", "pair_t", "pair_aff")] + [np.ascontiguousarray(rec[k], f32) for k in
                                                                                                  ("u", "v", "idepth_min", "idepth_max", "color", "weights", "energyTH")]
        A.nf, A.w, A.h, A.n, A.minObs = nf, w, h, ns, min_obs
        A.K[:] = [float(x) for x in win["K4"]]
        A.pair_R, A.pair_t, A.pair_aff = abi.fp(keep[0]), abi.fp(keep[1]), abi.fp(keep[2])
        A.u, A.v, A.idepth_min, A.idepth_max, A.color, A.weights, A.energyTH = [abi.fp(a) for a in keep[3:]]
        hosts = np.ascontiguousarray(rec["frame"], np.int32)
        A.host = abi.ip(hosts)
        imgs = [np.ascontiguousarray(i, f32) for i in win["imgs"]]
        ptrs = (abi.c_float_p * nf)(*[abi.fp(i) for i in imgs])
        A.dI = C.cast(ptrs, C.POINTER(abi.c_float_p))
        assert orc.orc_activate_points(C.byref(A), abi.ptr(status), abi.fp(idepth), abi.bp(res_state)) == 0
    rec.update(status=status, idepth=idepth, res_state=res_state)
    # ---- STEP 4
    flags = (dec == D.DELETE)
    flags[opt] = (status != 0) | (rec["lastTraceStatus"] == R.OOB)
    # ---- STEP 5
    for g in walked:
        fl = flags[frame == g]
        assert closed_form_order(fl) == R.remove_order(list(fl))
        R.remove(groups[g], fl)
    counts = np.zeros(abi.IMM_ACT_NCOUNTS, np.int32)
    counts[0] = n
    counts[1:4] = np.bincount(dec, minlength=3)[:3]
    counts[4] = ns
    counts[5:8] = [(status == s).sum() for s in (-1, 0, 1)]
    counts[8] = int(flags.sum())
    for f in range(nf):
        counts[9 + f] = 0 if groups[f] is None else len(groups[f]["u"])
    return dict(counts=counts, decision=dec, row=sel["row"], records=rec, frame=frame, index=index, flags=flags)
