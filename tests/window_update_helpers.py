"""What the sdso_ba_window_update tests share: the two paths to the edited window.
  path U: sdso_ba_window_update on the uploaded window;
  path F: the caller flattens the edited window by hand (the maps of tests/window_edit_ref.py, per-point / per-residual values from
          sdso_ba_get_post_state / sdso_ba_get_state of the old window, appended entries from the edit's payload) and uploads it fresh.
Windows are the dicts synth.ba_window returns (plus maxRelBaseline / numGoodResiduals / res_isNew once they have a history)."""
import ctypes as C

import numpy as np

from sdso_amd import abi
import window_edit_cases as cases
import window_edit_ref as ref

SLOT0 = 400                       # pyramid slot of a keyframe: SLOT0 + frameID


def with_history(win, seed):
    """the window with what earlier keyframes leave on it: depth priors on a part of the points, counts and baselines, residuals that are
    no longer new (the values sdso_ba_window_update has to carry for survivors)"""
    rs = np.random.RandomState(seed)
    w = dict(win)
    w["hasDepthPrior"] = (rs.rand(win["np"]) < 0.2).astype(np.uint8)
    w["numGoodResiduals"] = rs.randint(0, 9, win["np"]).astype(np.int32)
    w["maxRelBaseline"] = (rs.uniform(0, 0.4, win["np"]) * (rs.rand(win["np"]) < 0.7)).astype(np.float32)
    w["res_isNew"] = (rs.rand(win["nr"]) < 0.7).astype(np.uint8)
    return w


def slots(win):
    return [SLOT0 + int(f) for f in win["frameID"]]


def upload_pyramids(ctx, win, only=None):
    for f in range(win["nf"]):
        if only is None or f in only:
            ctx.upload_pyramid(SLOT0 + int(win["frameID"][f]), win["pyrs"][f][:1])


def make_window(win, with_images=False):
    return abi.make_ba_window(win, frame_slots=slots(win), dI_list=[p[0] for p in win["pyrs"]] if with_images else None)


def upload(ctx, win, wid):
    W, keep = make_window(win)
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid, C.byref(W)))
    return W, keep


def optimize(ctx, wid, its=6):
    out = abi.BAOptResult()
    ctx.check(ctx.L.sdso_ba_optimize(ctx.h, wid, its, None, None, None, C.byref(out)))
    return out


def post_state(ctx, wid, win):
    P, d = abi.make_post_state(win["nf"], win["np"], win["nr"])
    ctx.check(ctx.L.sdso_ba_get_post_state(ctx.h, wid, C.byref(P)))
    d = dict(d)
    d["calib_value_scaled"] = np.array(P.calib_value_scaled[:]); d["calib_value"] = np.array(P.calib_value[:]); d["calib_step"] = np.array(P.calib_step[:])
    d["counts"] = np.array([P.resInA, P.resInL, P.n_toRemove, P.result.iterations, P.result.resInA])
    d["energy"] = np.array([P.result.lastEnergy, P.result.rmse])
    d["resInM"] = np.array([P.resInM])
    return d


def assert_same(a, b, skip=(), what=""):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def values_from_post(win, d):
    """what the reference's objects hold after FullSystem::optimize, in the shape flatten() takes"""
    return dict(state=d["state"], state_zero=d["state_zero"], evalPT=d["evalPT"], frameEnergyTH=d["frameEnergyTH"],
                calib_value_scaled=d["calib_value_scaled"], idepth=d["idepth"], idepth_zero=d["idepth"],      # doStepFromBackup sets both
                maxRelBaseline=d["maxRelBaseline"], numGoodResiduals=d["numGoodResiduals"], res_state=d["state_state"])


def values_from_state(ctx, wid, win):
    """the same for a window that has not been optimised since its upload: what was uploaded, idepths and residual states as they stand"""
    st, idp, rs_ = np.zeros((win["nf"], 10)), np.zeros(win["np"], np.float32), np.zeros(win["nr"], np.uint8)
    ctx.check(ctx.L.sdso_ba_get_state(ctx.h, wid, abi.dp(st), abi.fp(idp), abi.bp(rs_)))
    npts = win["np"]
    return dict(state=st, state_zero=np.asarray(win["state_zero"]), evalPT=np.asarray(win["evalPT"]), frameEnergyTH=np.asarray(win["frameEnergyTH"]),
                calib_value_scaled=np.asarray(win["calib_value_scaled"]), idepth=idp, idepth_zero=np.asarray(win["idepth_zero"]),
                maxRelBaseline=np.asarray(win.get("maxRelBaseline", np.zeros(npts, np.float32))),
                numGoodResiduals=np.asarray(win.get("numGoodResiduals", np.zeros(npts, np.int32))), res_state=rs_)


def outlier_edit(win, d):
    """What FullSystem::optimize's callers do next: dropResidual for linearizeAll(true)'s toRemove in ascending window order
    (FullSystemOptimize.cpp:176-195), then removeOutliers: dropPointsF for the points left without a residual."""
    rem = np.nonzero(d["toRemove"])[0]
    left = np.bincount(win["res_point"][d["toRemove"] == 0], minlength=win["np"])
    return dict(drop_res=[int(r) for r in rem], drop_point=(left == 0).astype(np.uint8))


def _take(a, src, new):
    """rows of `a` through src (>= 0), rows of `new` where src = -1-k"""
    a = np.asarray(a)
    src = np.asarray(src, np.int64)
    out = np.zeros((len(src),) + a.shape[1:], a.dtype)
    old = src >= 0
    out[old] = a[src[old]]
    if (~old).any():
        out[~old] = np.asarray(new, a.dtype)[-1 - src[~old]]
    return np.ascontiguousarray(out)


def flatten(win, vals, edit, payload, maps=None, HM=None, bM=None):
    """The edited window, flattened by hand: (window dict, maps).  HM / bM: the prior of the edited window (default: zero)."""
    nf = win["nf"]
    maps = maps or ref.apply_edit(nf, win["host"], win["res_point"], win["res_target"], edit)
    frame_src, point_src, res_src = maps
    host2, rp2, rt2 = ref.flatten(nf, win["host"], win["res_point"], win["res_target"], edit, maps)
    af = payload.get("add_frames", {})
    ap = payload.get("add_points", {})
    n_ar = len(edit.get("add_res", []))
    nf2, np2, nr2 = len(frame_src), len(point_src), len(res_src)
    w2 = dict(win)
    w2.update(nf=nf2, np=np2, nr=nr2, host=host2, res_point=rp2, res_target=rt2)
    for k in ("evalPT", "state", "state_zero", "frameEnergyTH"):
        w2[k] = _take(vals[k], frame_src, af.get(k))
    for k in ("ab_exposure", "frameID"):
        w2[k] = _take(win[k], frame_src, af.get(k))
    w2["pyrs"] = [win["pyrs"][s] if s >= 0 else af["pyrs"][-1 - s] for s in frame_src]
    w2["calib_value_scaled"] = np.asarray(vals["calib_value_scaled"], np.float64)
    for k in ("u", "v", "color", "weights", "hasDepthPrior"):
        w2[k] = _take(win[k], point_src, ap.get(k))
    for k in ("idepth", "idepth_zero"):
        w2[k] = _take(vals[k], point_src, ap.get(k))
    n_ap = len(edit.get("add_points", []))
    w2["maxRelBaseline"] = _take(vals["maxRelBaseline"], point_src, ap.get("maxRelBaseline", np.zeros(n_ap, np.float32)))
    w2["numGoodResiduals"] = _take(vals["numGoodResiduals"], point_src, ap.get("numGoodResiduals", np.zeros(n_ap, np.int32)))
    new_state = np.concatenate([np.asarray(payload.get("add_res_state", np.zeros(n_ar)), np.uint8),
                                np.asarray(payload.get("pt_res_state", np.zeros(len(edit.get("pt_res", [])))), np.uint8)])
    w2["res_state"] = _take(vals["res_state"], res_src, new_state)
    old_new = np.asarray(win["res_isNew"], np.uint8) if win.get("res_isNew") is not None else np.ones(win["nr"], np.uint8)
    n_pr = len(edit.get("pt_res", []))
    new_isnew = np.concatenate([np.asarray(payload["add_res_isNew"], np.uint8) if payload.get("add_res_isNew") is not None else np.ones(n_ar, np.uint8),
                                np.asarray(payload["pt_res_isNew"], np.uint8) if payload.get("pt_res_isNew") is not None else np.ones(n_pr, np.uint8)])
    w2["res_isNew"] = _take(old_new, res_src, new_isnew)
    n2 = 8 * nf2 + 4
    w2["HM"] = np.zeros((n2, n2)) if HM is None else np.ascontiguousarray(HM, np.float64)
    w2["bM"] = np.zeros(n2) if bM is None else np.ascontiguousarray(bM, np.float64)
    w2.pop("idepth_true", None)
    return w2, maps


def update(ctx, wid, edit, payload=None):
    """path U; returns the call's status"""
    pl = dict(payload or {})
    if "add_frames" in pl:
        af = dict(pl["add_frames"])
        af["frame_slot"] = [SLOT0 + int(f) for f in af["frameID"]]
        pl["add_frames"] = af
    E, keep = cases.to_abi(edit, pl)
    return ctx.L.sdso_ba_window_update(ctx.h, wid, C.byref(E))


def get_order(ctx, wid, nf, npts, nr):
    fs, ps, rs_ = np.zeros(nf, np.int32), np.zeros(npts, np.int32), np.zeros(nr, np.int32)
    ctx.check(ctx.L.sdso_ba_window_get_order(ctx.h, wid, abi.ip(fs), abi.ip(ps), abi.ip(rs_)))
    return list(fs), list(ps), list(rs_)


def zero_extend(H, b, n2):
    """EnergyFunctional::insertFrame on HM / bM (EnergyFunctional.cpp:476-482)"""
    m = len(b)
    H2, b2 = np.zeros((n2, n2)), np.zeros(n2)
    H2[:m, :m] = np.asarray(H).reshape(m, m); b2[:m] = b
    return H2, b2


def snapshot(ctx, wid, win):
    """Every getter of a window that needs no optimize, then one linearize + applyRes + accumulate and what they leave"""
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    n = 8 * nf + 4
    L = ctx.L
    o = dict(state=np.zeros((nf, 10)), idepth=np.zeros(npts, np.float32), res_state=np.zeros(nr, np.uint8),
             precalc=np.zeros((nf * nf, 27), np.float32), adHost=np.zeros((nf * nf, 64)), adTarget=np.zeros((nf * nf, 64)), adHTdeltaF=np.zeros((nf * nf, 8), np.float32),
             cDeltaF=np.zeros(4, np.float32), frame_delta=np.zeros((nf, 8)), frame_delta_prior=np.zeros((nf, 8)), point_deltaF=np.zeros(npts, np.float32))
    ctx.check(L.sdso_ba_get_state(ctx.h, wid, abi.dp(o["state"]), abi.fp(o["idepth"]), abi.bp(o["res_state"])))
    ctx.check(L.sdso_ba_get_tables(ctx.h, wid, abi.fp(o["precalc"]), abi.dp(o["adHost"]), abi.dp(o["adTarget"]), abi.fp(o["adHTdeltaF"])))
    ctx.check(L.sdso_ba_get_deltas(ctx.h, wid, abi.fp(o["cDeltaF"]), abi.dp(o["frame_delta"]), abi.dp(o["frame_delta_prior"]), abi.fp(o["point_deltaF"])))
    e = C.c_double(0)
    ctx.check(L.sdso_ba_linearize(ctx.h, wid, C.byref(e)))
    o["energy"] = np.array([e.value])
    o.update(J=np.zeros((nr, 74), np.float32), newState=np.zeros(nr, np.uint8), newEnergy=np.zeros(nr, np.float32), newEnergyWO=np.zeros(nr, np.float32))
    ctx.check(L.sdso_ba_get_linearization(ctx.h, wid, abi.fp(o["J"]), abi.bp(o["newState"]), abi.fp(o["newEnergy"]), abi.fp(o["newEnergyWO"]), None, None))
    ctx.check(L.sdso_ba_apply_res(ctx.h, wid))
    o.update(state_after=np.zeros(nr, np.uint8), isActive=np.zeros(nr, np.uint8), JpJdF=np.zeros((nr, 8), np.float32))
    ctx.check(L.sdso_ba_get_residual_state(ctx.h, wid, abi.bp(o["state_after"]), abi.bp(o["isActive"]), abi.fp(o["JpJdF"])))
    ctx.check(L.sdso_ba_accumulate(ctx.h, wid))
    names = ("HdiF", "bdSumF", "Hdd_accAF", "bd_accAF")
    for k in names:
        o[k] = np.zeros(npts, np.float32)
    o["Hcd_accAF"] = np.zeros(npts * 4, np.float32)
    ctx.check(L.sdso_ba_get_point_terms(ctx.h, wid, *[abi.fp(o[k]) for k in names + ("Hcd_accAF",)]))
    o["accum"] = np.zeros(abi.accum_floats(nf), np.float32)
    ctx.check(L.sdso_ba_get_accumulators(ctx.h, wid, abi.fp(o["accum"])))
    st = [np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros(n)]
    ctx.check(L.sdso_ba_get_stitched(ctx.h, wid, *[abi.dp(a) for a in st]))
    for k, a in zip(("HA", "bA", "HL", "bL", "Hsc", "bsc"), st):
        o[k] = a
    return o


def marginalize_points(ctx, wid, win, flags):
    n = 8 * win["nf"] + 4
    HM, bM = np.zeros((n, n)), np.zeros(n)
    flags = np.ascontiguousarray(flags, np.uint8)
    ctx.check(ctx.L.sdso_ba_marginalize_points(ctx.h, wid, abi.bp(flags), abi.dp(HM), abi.dp(bM)))
    cnt = np.zeros(3, np.int32)
    ctx.check(ctx.L.sdso_ba_get_counts(ctx.h, wid, abi.ip(cnt[0:1]), abi.ip(cnt[1:2]), abi.ip(cnt[2:3])))
    return HM, bM, cnt


def marginalize_frame_dev(ctx, wid, idx, nf_left):
    m = 8 * nf_left + 4
    HM, bM = np.zeros((m, m)), np.zeros(m)
    ctx.check(ctx.L.sdso_ba_marginalize_frame_dev(ctx.h, wid, idx, abi.dp(HM), abi.dp(bM)))
    return HM, bM
