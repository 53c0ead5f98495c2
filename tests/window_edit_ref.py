"""The seven stages of sdso_ba_window_update as plain Python on lists of ids: the statement the C code is tested against.

A window is: per frame the list of its points (EFFrame::points), per point the list of its residuals (EFPoint::residualsAll).  Ids are
the indices of the window BEFORE the edit; appended entries get -1-k (frames, points; residuals: stage 6's first, then stage 7's).
Reference: EnergyFunctional::dropResidual (src/OptimizationBackend/EnergyFunctional.cpp:524-533), removePoint (:755-771),
dropPointsF (:739-752), marginalizePointsF's removePoint loop (:692-696), insertFrame (:462), insertResidual (:445), insertPoint (:507),
FullSystem::marginalizeFrame (src/FullSystem/FullSystemMarginalize.cpp:146-198); the resulting order is makeIDX's (:998-1018).

An edit is a dict with any of the keys
  drop_res [r...], remove_points [p...], drop_point [np flags], remove_frames [f...], n_add_frames k,
  add_res [(point, target)...], add_points [host...], pt_res [(index into add_points, target)...]
An edit the reference could not perform raises ValueError."""
import numpy as np

MAX_RES = 8


def _swap_out(lst, k):
    """what dropResidual / removePoint do to a std::vector: the LAST entry takes slot k, then pop_back"""
    lst[k] = lst[-1]
    lst.pop()


def remove_points_in_order(lst, leaving):
    """stage 2 on one host list: removePoint one after the other in the order of `leaving`"""
    lst = list(lst)
    for p in leaving:
        _swap_out(lst, lst.index(p))
    return lst


def drop_points_rescan(lst, leaving):
    """stage 3 on one host list: dropPointsF's loop `for i: if flagged: removePoint(p); i--`"""
    lst = list(lst)
    leaving = set(leaving)
    i = 0
    while i < len(lst):
        if lst[i] in leaving:
            _swap_out(lst, i)
        else:
            i += 1
    return lst


def apply_edit(nf, host, res_point, res_target, edit):
    """Returns (frame_src, point_src, res_src) as lists."""
    host = [int(h) for h in host]
    res_point = [int(p) for p in res_point]
    res_target = [int(t) for t in res_target]
    npts, nr = len(host), len(res_point)
    k_add = int(edit.get("n_add_frames", 0))
    frames = list(range(nf))                                     # ids in window order
    pts = {f: [p for p in range(npts) if host[p] == f] for f in range(nf)}
    res = {p: [] for p in range(npts)}
    for r in range(nr):
        res[res_point[r]].append(r)
    p_alive, r_alive = set(range(npts)), set(range(nr))

    def need(cond, why):
        if not cond:
            raise ValueError(why)

    def remove_point(p):
        for r in res[p]:
            r_alive.discard(r)
        res[p] = []
        _swap_out(pts[host[p]], pts[host[p]].index(p))
        p_alive.discard(p)

    # stage 1
    for r in edit.get("drop_res", []):
        r = int(r)
        need(0 <= r < nr and r in r_alive, "stage 1")
        l = res[res_point[r]]
        _swap_out(l, l.index(r))
        r_alive.discard(r)
    # stage 2
    for p in edit.get("remove_points", []):
        p = int(p)
        need(0 <= p < npts and p in p_alive, "stage 2")
        remove_point(p)
    # stage 3
    flags = edit.get("drop_point")
    if flags is not None:
        need(len(flags) == npts and all(p in p_alive for p in range(npts) if flags[p]), "stage 3")
        for f in frames:
            i = 0
            while i < len(pts[f]):
                if flags[pts[f][i]]:
                    remove_point(pts[f][i])
                else:
                    i += 1
    # stage 4
    for f in edit.get("remove_frames", []):
        f = int(f)
        need(0 <= f < nf and f in frames and not pts[f], "stage 4")
        for p in sorted(p_alive):
            for k, r in enumerate(res[p]):
                if res_target[r] == f:
                    _swap_out(res[p], k)
                    r_alive.discard(r)
                    break
        frames.remove(f)
    # stage 5
    for k in range(k_add):
        frames.append(nf + k)
        pts[nf + k] = []
    need(1 <= len(frames) <= 8, "stage 5")
    # stage 6
    add_res = [(int(p), int(t)) for p, t in edit.get("add_res", [])]

    def target_of(rid):
        return res_target[rid] if rid >= 0 else add_res[-1 - rid][1]
    for k, (p, t) in enumerate(add_res):
        need(0 <= p < npts and p in p_alive and t in frames and t != host[p], "stage 6")
        need(all(target_of(r) != t for r in res[p]) and len(res[p]) < MAX_RES, "stage 6")
        res[p].append(-1 - k)
    # stage 7
    add_pts = [int(h) for h in edit.get("add_points", [])]
    pt_res = [(int(q), int(t)) for q, t in edit.get("pt_res", [])]
    new_res = {q: [] for q in range(len(add_pts))}
    for q, h in enumerate(add_pts):
        need(h in frames, "stage 7")
        pts[h].append(-1 - q)
    last = 0
    for k, (q, t) in enumerate(pt_res):
        need(last <= q < len(add_pts) and t in frames and t != add_pts[q], "stage 7")
        need(all(pt_res[-1 - r - len(add_res)][1] != t for r in new_res[q]) and len(new_res[q]) < MAX_RES, "stage 7")
        new_res[q].append(-1 - (len(add_res) + k))
        last = q
    # makeIDX
    frame_src = [f if f < nf else -1 - (f - nf) for f in frames]
    point_src, res_src = [], []
    for f in frames:
        for p in pts[f]:
            point_src.append(p)
            res_src += res[p] if p >= 0 else new_res[-1 - p]
    return frame_src, point_src, res_src


def flatten(nf, host, res_point, res_target, edit, maps):
    """host / res_point / res_target of the edited window in its own numbering, from the maps apply_edit returned"""
    frame_src, point_src, res_src = maps
    old_frame = [f if f >= 0 else nf + (-1 - f) for f in frame_src]
    fnew = {f: i for i, f in enumerate(old_frame)}
    add_res = list(edit.get("add_res", []))
    add_pts = list(edit.get("add_points", []))
    pt_res = list(edit.get("pt_res", []))
    host2 = [fnew[int(host[p])] if p >= 0 else fnew[int(add_pts[-1 - p])] for p in point_src]
    pnew = {p: i for i, p in enumerate(point_src)}
    rp, rt = [], []
    for r in res_src:
        if r >= 0:
            rp.append(pnew[int(res_point[r])]); rt.append(fnew[int(res_target[r])])
        elif -1 - r < len(add_res):
            rp.append(pnew[int(add_res[-1 - r][0])]); rt.append(fnew[int(add_res[-1 - r][1])])
        else:
            q, t = pt_res[-1 - r - len(add_res)]
            rp.append(pnew[-1 - int(q)]); rt.append(fnew[int(t)])
    return np.array(host2, np.int32), np.array(rp, np.int32), np.array(rt, np.int32)
