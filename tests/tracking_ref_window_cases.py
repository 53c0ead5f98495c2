"""Windows for sdso_track_make_ref_from_window and the route it replaces, stated once for the GPU tests and tools/time_tracking_ref.py.

make_case      a synth.ba_window whose residual lists went through dropResidual (helpers.drop_residuals), with a noisy idepth so that
               FullSystem::optimize leaves OUTLIER / toRemove residuals behind, and the right image of its newest keyframe.
with_triples   the same window with some points present three times (the copies' idepth differs by a relative 1e-4): three points on
               one pixel of the newest keyframe, where STEP1's += depends on the order (CoarseTracker.cpp:352-354).
host_route     the route of sdso_shim::CoarseTracker::setCoarseTrackingRef(frameHessians, fh_right, Hcalib): sdso_ba_get_post_state,
               the gather on the host, sdso_stereo_match_batch, the accept rule (:329-341), sdso_track_make_ref.
window_route   sdso_track_make_ref_from_window and its per-point records."""
import ctypes as C

import numpy as np

import helpers
from sdso_amd import abi
import synth
from tracking_ref_window_ref import expected_points

KEYS = ("u", "v", "idepth", "color")


def make_case(w=320, h=240, nf=4, pts_per_kf=200, seed=3101, idepth_noise=0.2, drop_seed=5, drop_frac=0.15, scene_seed=1001):
    win = synth.ba_window(w=w, h=h, nf=nf, pts_per_kf=pts_per_kf, seed=seed, idepth_noise=idepth_noise, scene_seed=scene_seed)
    if drop_frac > 0:
        win, _ = helpers.drop_residuals(win, seed=drop_seed, drop_frac=drop_frac)
    return add_right(win, seed, scene_seed)


def add_right(win, seed, scene_seed=1001):
    """the right camera of the newest keyframe: its pose shifted by the baseline, as synth.stereo_problem places it"""
    R, t = win["poses"][-1]
    bl = float(win["calib"]["baseline"])
    img, _ = synth.Scene(scene_seed).render(win["w"], win["h"], win["K"], (R, t + np.array([-bl, 0.0, 0.0])), noise_seed=seed + 777, aff=win["affs"][-1])
    out = dict(win)
    out["pyr_right"] = synth.make_pyramid(img, win["levels"])
    out["baseline"] = bl
    return out


def with_triples(win, every=5):
    """every `every`-th point that observes the newest keyframe twice more, right behind itself in its host's group, with its residuals"""
    starts = np.searchsorted(win["res_point"], np.arange(win["np"]), side="left")
    ends = np.searchsorted(win["res_point"], np.arange(win["np"]), side="right")
    src, scale = [], []
    cand = 0
    for p in range(win["np"]):
        src.append(p); scale.append(1.0)
        if (win["res_target"][starts[p]:ends[p]] == win["nf"] - 1).any():
            if cand % every == 0:
                src += [p, p]; scale += [1.0 + 1e-4, 1.0 - 1e-4]
            cand += 1
    src = np.array(src); scale = np.array(scale, np.float32)
    out = dict(win)
    for k in ("u", "v", "color", "weights", "host", "hasDepthPrior", "idepth_true"):
        out[k] = np.ascontiguousarray(win[k][src])
    for k in ("idepth", "idepth_zero"):
        out[k] = (win[k][src] * scale).astype(np.float32)
    rp, ridx = [], []
    for pn, po in enumerate(src):
        rp += [pn] * int(ends[po] - starts[po])
        ridx += list(range(int(starts[po]), int(ends[po])))
    out["res_point"] = np.array(rp, np.int32)
    for k in ("res_target", "res_state"):
        out[k] = np.ascontiguousarray(win[k][ridx])
    out["np"], out["nr"] = len(src), len(rp)
    out["triple_src"] = src
    return out


def upload(ctx, case, wid, slot0):
    """pyramids (all levels: the newest keyframe's carry the template) into slot0 .. slot0 + nf - 1, the right image into slot0 + nf"""
    nf = case["nf"]
    for f in range(nf):
        ctx.upload_pyramid(slot0 + f, case["pyrs"][f])
    ctx.upload_pyramid(slot0 + nf, case["pyr_right"])
    W, keep = abi.make_ba_window(case, frame_slots=[slot0 + f for f in range(nf)], dI_list=[p[0] for p in case["pyrs"]])
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid, C.byref(W)))
    return dict(wid=wid, left=slot0 + nf - 1, right=slot0 + nf, baseline=case["baseline"], W=W, keep=keep)


def optimize(ctx, wid, its=3):
    out = abi.BAOptResult()
    ctx.check(ctx.L.sdso_ba_optimize(ctx.h, wid, its, None, None, None, C.byref(out)))
    return out


def post_state(ctx, case, wid, projections=True):
    P, d = abi.make_post_state(case["nf"], case["np"], case["nr"], with_system=False)
    if not projections:
        P.centerProjectedTo = None; P.projectedTo = None
    ctx.check(ctx.L.sdso_ba_get_post_state(ctx.h, wid, C.byref(P)))
    d["K32"] = np.array(P.calib_value_scaled[:], np.float64).astype(np.float32)     # Hcalib.fxl() .. cyl(): value_scaledf
    return d


def get_ref(ctx, slot, levels):
    out = []
    for l in range(levels):
        nn = C.c_int(-1)
        ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), None, None, None, None))
        arrs = [np.zeros(nn.value, np.float32) for _ in KEYS]
        if nn.value:
            ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), *[abi.fp(a) for a in arrs]))
        out.append(dict(zip(KEYS, arrs)))
    return out


def gather_host(case, post, order=None):
    """STEP1's loop on the host (CoarseTracker.cpp:295-312, :350) over the downloaded post-state -> the chain's inputs, in splat order"""
    pts = expected_points(post["state_state"], post["isActiveAndIsGoodNEW"], case["res_target"], case["res_point"], case["nf"] - 1, order, case["np"])
    res_of = np.full(case["np"], -1, np.int64)
    newest = np.nonzero(case["res_target"] == case["nf"] - 1)[0]
    res_of[case["res_point"][newest]] = newest
    cpt = post["centerProjectedTo"][res_of[pts]]
    ui = (cpt[:, 0] + np.float32(0.5)).astype(np.int32)
    vi = (cpt[:, 1] + np.float32(0.5)).astype(np.int32)
    weight = np.sqrt((1e-3 / (post["HdiF"][pts].astype(np.float64) + 1e-12)).astype(np.float32)).astype(np.float32)
    return dict(point=pts, u=ui, v=vi, cpt2=np.ascontiguousarray(cpt[:, 2]), weight=weight,
                imin=(cpt[:, 2] * np.float32(0.1)).astype(np.float32), imax=(cpt[:, 2] * np.float32(1.9)).astype(np.float32))


def host_route(ctx, case, up, ref_slot, order=None, post=None, clock=None):
    """-> (STEP1 arrays in splat order, pc_n); installs the reference in ref_slot.  clock: a list that receives perf_counter() after the
    post-state, the gather, the match, the accept rule and sdso_track_make_ref (tools/time_tracking_ref.py)"""
    import time
    tick = (lambda: clock.append(time.perf_counter())) if clock is not None else (lambda: None)
    post = post_state(ctx, case, up["wid"]) if post is None else post
    tick()
    g = gather_host(case, post, order)
    tick()
    n = len(g["point"])
    uf, vf = g["u"].astype(np.float32), g["v"].astype(np.float32)
    sf, sb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ids, buv = np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
    if n:
        M = abi.StereoMatch()
        M.n = n; M.u = abi.fp(uf); M.v = abi.fp(vf)
        M.idepth_min_stereo = abi.fp(g["imin"]); M.idepth_max_stereo = abi.fp(g["imax"])
        M.back_idepth_min_stereo = abi.fp(g["imin"]); M.back_idepth_max_stereo = abi.fp(g["imax"])
        M.status_fwd = abi.bp(sf); M.status_back = abi.bp(sb); M.idepth_stereo = abi.fp(ids); M.back_uv = abi.fp(buv)
        ctx.check(ctx.L.sdso_stereo_match_batch(ctx.h, up["left"], up["right"], abi.fp(post["K32"]), case["baseline"], 1, C.byref(M)))
    tick()
    new_idepth = g["cpt2"].copy()
    good = np.nonzero(sf == 0)[0]
    with np.errstate(divide="ignore"):
        depth = np.float32(1.0) / ids[good]
    ok = (np.abs(uf[good] - buv[good, 0]) < 1) & (depth > 0) & (depth < 50)
    new_idepth[good[ok]] = ids[good[ok]]
    tick()
    pcn = np.zeros(8, np.int32)
    ctx.check(ctx.L.sdso_track_make_ref(ctx.h, ref_slot, up["left"], n, abi.ip(g["u"]), abi.ip(g["v"]), abi.fp(new_idepth), abi.fp(g["weight"]), abi.ip(pcn)))
    tick()
    g.update(status_fwd=sf, status_back=sb, new_idepth=new_idepth, n_stereo=int(ok.sum()))
    return g, pcn


def window_call(ctx, up, ref_slot, order=None, right=None, want=True):
    """sdso_track_make_ref_from_window -> (return code, n_points, n_border, pc_n)"""
    npts, nb, pcn = C.c_int(-1), C.c_int(-1), np.full(8, -1, np.int32)
    o = None if order is None else np.ascontiguousarray(order, np.int32)
    rc = ctx.L.sdso_track_make_ref_from_window(ctx.h, ref_slot, up["wid"], up["right"] if right is None else right, up["baseline"],
                                               None if o is None else abi.ip(o), 0 if o is None else len(o),
                                               C.byref(npts) if want else None, C.byref(nb) if want else None, abi.ip(pcn) if want else None)
    return rc, npts.value, nb.value, pcn


def ref_points(ctx, ref_slot):
    nn = C.c_int(-1)
    ctx.check(ctx.L.sdso_track_get_ref_points(ctx.h, ref_slot, C.byref(nn), None, None, None, None, None, None, None, None))
    n = nn.value
    d = dict(point=np.zeros(n, np.int32), u=np.zeros(n, np.int32), v=np.zeros(n, np.int32), cpt2=np.zeros(n, np.float32),
             status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), new_idepth=np.zeros(n, np.float32), weight=np.zeros(n, np.float32))
    ctx.check(ctx.L.sdso_track_get_ref_points(ctx.h, ref_slot, C.byref(nn), abi.ip(d["point"]), abi.ip(d["u"]), abi.ip(d["v"]), abi.fp(d["cpt2"]),
                                              abi.bp(d["status_fwd"]), abi.bp(d["status_back"]), abi.fp(d["new_idepth"]), abi.fp(d["weight"])))
    return d


def window_route(ctx, up, ref_slot, order=None):
    rc, npts, nb, pcn = window_call(ctx, up, ref_slot, order)
    ctx.check(rc)
    d = ref_points(ctx, ref_slot)
    assert len(d["point"]) == npts
    return d, pcn, nb


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
