"""Seeded random, LEGAL edits for sdso_ba_window_plan / sdso_ba_window_update, and the marshalling of an edit dict (window_edit_ref)
into the ABI structure.  Legality is decided on the lists the model leaves after stages 1-4 (which points survive, what they observe);
the order the edit produces is never taken from here."""
import numpy as np

import window_edit_ref as ref


def lists_after_removals(nf, host, res_point, res_target, edit):
    """(surviving frames, surviving points, {point: targets it still observes}) after stages 1-4 of `edit`"""
    part = {k: edit[k] for k in ("drop_res", "remove_points", "drop_point", "remove_frames") if k in edit}
    frame_src, point_src, res_src = ref.apply_edit(nf, host, res_point, res_target, part)
    obs = {p: [] for p in point_src}
    for r in res_src:
        obs[int(res_point[r])].append(int(res_target[r]))
    return frame_src, point_src, obs


def random_edit(rs, nf, host, res_point, res_target, res_frac=0.15, marg_frac=0.08, drop_frac=0.08, remove_frames=(), n_add_frames=0,
                add_res_frac=0.3, n_add_points=0, shuffle_drops=False, empty_host=None):
    host = np.asarray(host); res_point = np.asarray(res_point); res_target = np.asarray(res_target)
    npts, nr = len(host), len(res_point)
    edit = {}
    dr = np.nonzero(rs.rand(nr) < res_frac)[0]
    if shuffle_drops:
        dr = rs.permutation(dr)
    edit["drop_res"] = [int(r) for r in dr]
    sel = rs.rand(npts)
    leaving_hosts = set(int(f) for f in remove_frames)
    marg = [int(p) for p in rs.permutation(npts) if sel[p] < marg_frac or (int(host[p]) in leaving_hosts and sel[p] < 0.5)]
    edit["remove_points"] = marg
    flags = ((sel >= marg_frac) & (sel < marg_frac + drop_frac)).astype(np.uint8)
    for p in range(npts):                                         # a frame that leaves, or `empty_host`, loses every point
        if int(host[p]) in leaving_hosts or int(host[p]) == empty_host:
            flags[p] = 1
    flags[marg] = 0
    edit["drop_point"] = flags
    edit["remove_frames"] = [int(f) for f in remove_frames]
    edit["n_add_frames"] = int(n_add_frames)
    frames, points, obs = lists_after_removals(nf, host, res_point, res_target, edit)
    alive = list(frames) + [nf + k for k in range(n_add_frames)]
    add_res = []
    for p in points:
        if rs.rand() < add_res_frac:
            free = [t for t in alive if t != int(host[p]) and t not in obs[p]]
            take = list(rs.permutation(free)[:max(0, min(len(free), ref.MAX_RES - len(obs[p]), 1 + rs.randint(2)))])
            for t in take:
                add_res.append((int(p), int(t)))
                obs[p].append(int(t))
    order = rs.permutation(len(add_res))
    edit["add_res"] = [add_res[i] for i in order]                 # (any order across points; per point the order is the push order)
    hosts = [int(alive[rs.randint(len(alive))]) for _ in range(n_add_points)]
    pt_res = []
    for q, h in enumerate(hosts):
        others = [t for t in alive if t != h]
        for t in rs.permutation(others)[:rs.randint(0, min(len(others), ref.MAX_RES) + 1)]:
            pt_res.append((q, int(t)))
    edit["add_points"] = hosts
    edit["pt_res"] = pt_res
    return edit


def to_abi(edit, payload=None):
    """abi.make_window_edit arguments from an edit dict; payload: dict(add_frames=..., add_res_state, add_res_isNew, add_points={...
    per-point arrays ...}, pt_res_state, pt_res_isNew) for sdso_ba_window_update (the plan needs none: zeros are filled in)."""
    from sdso_amd import abi
    payload = payload or {}
    k = int(edit.get("n_add_frames", 0))
    add_frames = payload.get("add_frames")
    if k and add_frames is None:
        add_frames = dict(evalPT=np.zeros((k, 12)), state=np.zeros((k, 10)), state_zero=np.zeros((k, 10)), ab_exposure=np.ones(k, np.float32),
                          frameEnergyTH=np.ones(k, np.float32), frameID=np.arange(100, 100 + k), frame_slot=np.zeros(k, np.int32))
    ar = list(edit.get("add_res", []))
    add_res = None
    if ar:
        add_res = dict(point=[p for p, _ in ar], target=[t for _, t in ar], state=payload.get("add_res_state", np.zeros(len(ar), np.uint8)),
                       isNew=payload.get("add_res_isNew"))
    ap = list(edit.get("add_points", []))
    add_points = None
    if ap:
        n = len(ap)
        pr = list(edit.get("pt_res", []))
        add_points = dict(host=ap, u=np.zeros(n), v=np.zeros(n), idepth=np.zeros(n), idepth_zero=np.zeros(n), color=np.zeros((n, 8)),
                          weights=np.zeros((n, 8)), hasDepthPrior=np.zeros(n, np.uint8))
        add_points.update(payload.get("add_points", {}))
        add_points.update(res_point=[q for q, _ in pr], res_target=[t for _, t in pr],
                          res_state=payload.get("pt_res_state", np.zeros(len(pr), np.uint8)), res_isNew=payload.get("pt_res_isNew"))
    return abi.make_window_edit(drop_res=edit.get("drop_res"), remove_points=edit.get("remove_points"), drop_point=edit.get("drop_point"),
                                remove_frames=edit.get("remove_frames"), add_frames=add_frames if k else None, add_res=add_res,
                                add_points=add_points)


def c_plan(nf, host, res_point, res_target, edit):
    """sdso_ba_window_plan: (rc, frame_src, point_src, res_src)"""
    import ctypes as C
    from sdso_amd import abi
    L = abi.load()
    host = np.ascontiguousarray(host, np.int32); rp = np.ascontiguousarray(res_point, np.int32); rt = np.ascontiguousarray(res_target, np.int32)
    E, keep = to_abi(edit)
    n2 = [C.c_int(-7) for _ in range(3)]
    fs = np.full(nf + E.n_add_frames, -99, np.int32)
    ps = np.full(len(host) + E.n_add_points, -99, np.int32)
    rsrc = np.full(len(rp) + E.n_add_res + E.n_pt_res, -99, np.int32)
    rc = L.sdso_ba_window_plan(nf, len(host), len(rp), abi.ip(host), abi.ip(rp), abi.ip(rt), C.byref(E), C.byref(n2[0]), C.byref(n2[1]), C.byref(n2[2]),
                               abi.ip(fs), abi.ip(ps), abi.ip(rsrc))
    if rc != 0:
        return rc, None, None, None
    return rc, list(fs[:n2[0].value]), list(ps[:n2[1].value]), list(rsrc[:n2[2].value])
