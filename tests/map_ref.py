"""KeyFrameDisplay::setFromKF / refreshPC restated in numpy, float32 throughout with the one double quotient: the reference of
sdso_map_update / sdso_map_cloud, the two walking loops that turn removal decisions into list orders, and the cases their tests run on.

Reference: IOWrapper/Pangolin/KeyFrameDisplay.cpp:68-83 (setFromF), :85-165 (setFromKF), :174-295 (refreshPC);
FullSystemOptimize.cpp:1063-1084 (removeOutliers: swap-with-back while walking), FullSystem.cpp:990-1053 (flagPointsForRemoval: null,
then compact with swap-with-back).  Written from those lines — it shares no code with csrc/map_cloud.h.

Deviations of the library, followed here: z = depth (the rand() jitter of :246 at its mean) and no sparsification (:240)."""
import numpy as np

import flag_points_ref as fref

F = np.float32
REC = 16                                          # u, v, idepth, idepth_hessian, maxRelBaseline, color[8], 3 x padding
IMMATURE, ACTIVE, MARGINALIZED, OUT = 0, 1, 2, 3  # InputPointSparse::status (:115, :129, :144, :158)
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))   # patternP = staticPattern[8], settings.cpp:216
MODE0_COLOURS = {IMMATURE: (0, 255, 255), ACTIVE: (0, 255, 0), MARGINALIZED: (0, 0, 255), OUT: (255, 0, 0)}   # :252-275

# The windows of tests/flag_points_ref.py with, on the CPU oracle's post-state and the quantile thresholds below in mode 1: the points
# each clause drops (mode / scaled / abs / bs, in the order the clauses are tested), the points kept, and the status counts (1 / 2 / 3)
CASES = {"A": dict(dropped=(134, 56, 26, 9), kept=95, status=(105, 81, 134)),
         "B": dict(dropped=(295, 92, 38, 11), kept=164, status=(197, 108, 295)),
         "C": dict(dropped=(143, 29, 13, 5), kept=50, status=(59, 38, 143))}
ORDER_SEED = 77                                   # the permutation of fh->pointHessians inside every host


# ------------------------------------------------------------------ the lists
def records_from_post(win, post, idx):
    """setFromKF's record (:121-129) of the window points idx, from what sdso_ba_get_post_state returns: [len(idx), 16] float32"""
    idx = np.asarray(idx, np.int64)
    r = np.zeros((len(idx), REC), F)
    r[:, 0] = np.asarray(win["u"], F)[idx]
    r[:, 1] = np.asarray(win["v"], F)[idx]
    r[:, 2] = np.asarray(post["idepth"], F)[idx]                  # idepth_scaled, SCALE_IDEPTH = 1
    r[:, 3] = np.asarray(post["idepth_hessian"], F)[idx]
    r[:, 4] = np.asarray(post["maxRelBaseline"], F)[idx]
    r[:, 5:13] = np.asarray(win["color"], F).reshape(-1, 8)[idx]
    return r


def immature_records(u, v, idepth_min, idepth_max, color):
    """:104-117"""
    n = len(u)
    r = np.zeros((n, REC), F)
    r[:, 0] = u; r[:, 1] = v
    with np.errstate(invalid="ignore"):
        r[:, 2] = (np.asarray(idepth_max, F) + np.asarray(idepth_min, F)) * F(0.5)
    r[:, 3] = 1000; r[:, 4] = 0
    r[:, 5:13] = np.asarray(color, F).reshape(n, 8)
    return r


def point_lists(host, nf, seed=ORDER_SEED):
    """fh->pointHessians of every frame as window point indices: a seeded permutation inside each host, so that the list order differs
    from the window's"""
    rs = np.random.RandomState(seed)
    host = np.asarray(host)
    return [[int(p) for p in rs.permutation(np.nonzero(host == h)[0])] for h in range(nf)]


def walk_remove_outliers(lists, no_residual):
    """FullSystemOptimize.cpp:1066-1081 on every frame: (lists after it, the points pushed to pointHessiansOut in push order)"""
    out, pushed = [], []
    for ph in lists:
        ph = list(ph)
        i = 0
        while i < len(ph):
            if no_residual[ph[i]]:
                pushed.append(ph[i])                  # :1074
                ph[i] = ph[-1]                        # :1076
                ph.pop()                              # :1077
                i -= 1                                # :1078
            i += 1
        out.append(ph)
    return out, pushed


def walk_flag_points(lists, decision):
    """FullSystem.cpp:990-1053 on every frame: (lists after it, the points pushed in push order, the list each went to: 2 / 3)"""
    out, pushed, where = [], [], []
    for ph in lists:
        ph = list(ph)
        for i in range(len(ph)):
            d = decision[ph[i]]
            if d == fref.KEEP:
                continue
            pushed.append(ph[i])
            where.append(MARGINALIZED if d == fref.MARGINALIZE else OUT)           # :1026-1040
            ph[i] = None                                                           # :1043
        i = 0
        while i < len(ph):                                                         # :1047-1053
            if ph[i] is None:
                ph[i] = ph[-1]
                ph.pop()
                i -= 1
            i += 1
        out.append(ph)
    return out, pushed, where


def walk(lists, decision):
    """removeOutliers, then flagPointsForRemoval, from the decisions of sdso_ba_flag_points: what sdso_map_update takes.
    Returns dict: active (list per frame), gone, gone_list"""
    decision = np.asarray(decision)
    l1, g1 = walk_remove_outliers(lists, decision == fref.DROP_NO_RESIDUAL)
    d2 = decision.copy()
    l2, g2, w2 = walk_flag_points(l1, d2)
    assert not set(g1) & set(g2)
    return dict(active=l2, gone=np.array(g1 + g2, np.int32), gone_list=np.array([OUT] * len(g1) + w2, np.uint8))


def lists_after(win, post, w, before=None):
    """The three lists of every keyframe after an update with walk() result w: {frameID: {1: records, 2: records, 3: records}}.
    before: the lists the map held (marginalised and out are appended to, active is replaced)."""
    host = np.asarray(win["host"])
    res = {}
    for h in range(win["nf"]):
        fid = int(win["frameID"][h])
        old = (before or {}).get(fid, {})
        g, gl = w["gone"], w["gone_list"]
        mine = host[g] == h if len(g) else np.zeros(0, bool)
        new = {ACTIVE: records_from_post(win, post, w["active"][h])}
        for lst in (MARGINALIZED, OUT):
            add = records_from_post(win, post, g[mine & (gl == lst)])
            new[lst] = np.concatenate([old[lst], add]) if lst in old else add
        res[fid] = new
    for fid, l in (before or {}).items():
        res.setdefault(fid, l)
    return res


# ------------------------------------------------------------------ refreshPC
def inverse_calib(K4):
    """:77-80, float"""
    fx, fy, cx, cy = [F(x) for x in K4]
    return F(1) / fx, F(1) / fy, -cx / fx, -cy / fy


def drop_clause(status, rec, mode, scaledTH, absTH, minBS):
    """:215-234 per record: 0 kept, 1 mode / status, 2 negative idepth, 3 scaled, 4 abs, 5 baseline.  Also returns (var, var * depth^4)."""
    status = np.asarray(status)
    idepth, idh, bs = rec[:, 2], rec[:, 3], rec[:, 4]
    with np.errstate(all="ignore"):
        depth = F(1) / idepth                                             # :222
        depth4 = depth * depth                                            # :223
        depth4 = depth4 * depth4                                          # :224
        var = (1.0 / (idh.astype(np.float64) + 0.01)).astype(F)           # :225: 0.01 is a double
        scaled = var * depth4
        c = np.zeros(len(rec), np.int32)
        if mode == 1:
            m = (status != ACTIVE) & (status != MARGINALIZED)
        elif mode == 2:
            m = status != ACTIVE
        else:
            m = np.full(len(rec), mode > 2)
        tests = ((1, m), (2, idepth < 0), (3, scaled > F(scaledTH)), (4, var > F(absTH)), (5, bs < F(minBS)))
        for code, t in tests:
            c[(c == 0) & t] = code
    return c, var, scaled


def grey(c):
    """(unsigned char)c as the reference's x86 build converts: float -> int truncating (INT_MIN for a NaN or a value outside int), low byte"""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(c) & (c >= F(-2 ** 31)) & (c < F(2 ** 31))
    i = np.where(ok, np.trunc(np.where(ok, c, 0)).astype(np.int64), -2 ** 31)
    return (i & 0xFF).astype(np.uint8)


def quantile_thresholds(frames):
    """The thresholds of the tests: over the mode-1 candidates (status 1 or 2) with idepth >= 0 of all frames, scaledTH = the 0.7-quantile
    of var * depth^4, absTH = the 0.7-quantile of var, minBS = the 0.3-quantile of maxRelBaseline; float32"""
    rec = np.concatenate([f["lists"][l] for f in frames for l in (ACTIVE, MARGINALIZED)])
    rec = rec[rec[:, 2] >= 0]
    _, var, scaled = drop_clause(np.full(len(rec), ACTIVE), rec, 1, np.inf, np.inf, -np.inf)
    return dict(scaledTH=float(F(np.quantile(scaled.astype(np.float64), 0.7))), absTH=float(F(np.quantile(var.astype(np.float64), 0.7))),
                minBS=float(F(np.quantile(rec[:, 4].astype(np.float64), 0.3))))


def cloud(frames, K4, scaledTH=0.001, absTH=0.001, minBS=0.1, mode=1, camToWorld=None):
    """refreshPC over frames = [dict(lists={1: rec, 2: rec, 3: rec}, imm=rec or None)], packed in the order frame / immature, active,
    marginalised, out / list order / pattern.  Returns dict: xyz [n, 3] float32, rgb [n, 3] uint8, first [n_frames + 1], kept [n_frames, 4]
    (points), clause (per record, in input order)."""
    fxi, fyi, cxi, cyi = inverse_calib(K4)
    xyz, rgb, first, kept, clauses = [], [], [0], np.zeros((len(frames), 4), np.int32), []
    nv = 0
    for k, fr in enumerate(frames):
        for st in (IMMATURE, ACTIVE, MARGINALIZED, OUT):
            rec = fr.get("imm") if st == IMMATURE else fr["lists"][st]
            if rec is None or len(rec) == 0:
                continue
            c, _, _ = drop_clause(np.full(len(rec), st), rec, mode, scaledTH, absTH, minBS)
            clauses.append(c)
            r = rec[c == 0]
            kept[k, st] = len(r)
            if not len(r):
                continue
            with np.errstate(all="ignore"):
                depth = F(1) / r[:, 2]
                V = np.zeros((len(r), 8, 3), F)
                Cb = np.zeros((len(r), 8, 3), np.uint8)
                for p, (dx, dy) in enumerate(PATTERN):
                    x = ((r[:, 0] + F(dx)) * fxi + cxi) * depth                   # :244
                    y = ((r[:, 1] + F(dy)) * fyi + cyi) * depth                   # :245
                    z = depth                                                     # :246 without the jitter
                    if camToWorld is not None:
                        T = np.asarray(camToWorld, F).reshape(-1, 12)[k]
                        x, y, z = [T[3 * i] * x + T[3 * i + 1] * y + T[3 * i + 2] * z + T[9 + i] for i in range(3)]
                    V[:, p, 0], V[:, p, 1], V[:, p, 2] = x, y, z
                    Cb[:, p, :] = np.array(MODE0_COLOURS[st], np.uint8) if mode == 0 else grey(r[:, 5 + p])[:, None]   # :250-289
            xyz.append(V.reshape(-1, 3)); rgb.append(Cb.reshape(-1, 3))
            nv += 8 * len(r)
        first.append(nv)
    return dict(xyz=np.concatenate(xyz) if xyz else np.zeros((0, 3), F), rgb=np.concatenate(rgb) if rgb else np.zeros((0, 3), np.uint8),
                first=np.array(first, np.int32), kept=kept, clause=np.concatenate(clauses) if clauses else np.zeros(0, np.int32))


def assert_cloud_equal(got, want, what=""):
    """bit patterns and bytes; a NaN vertex compares as "NaN in the same place" """
    n = int(want["first"][-1])
    assert np.array_equal(got["first"], want["first"]), (what, got["first"], want["first"])
    assert np.array_equal(got["kept"], want["kept"]), (what, got["kept"], want["kept"])
    g, w = np.ascontiguousarray(got["xyz"][:n]), np.ascontiguousarray(want["xyz"])
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    gb, wb = g.view(np.uint32), w.view(np.uint32)
    assert np.array_equal(gb[~nan], wb[~nan]), (what, np.argwhere((gb != wb) & ~nan)[:5])
    assert np.array_equal(got["rgb"][:n], want["rgb"]), (what, np.argwhere(got["rgb"][:n] != want["rgb"])[:5])


def case_on_post(name, win, post, frame_marg, last_gone):
    """What both the oracle test and the GPU test do with a window and a post-state: decisions, the walk, the lists of every keyframe.
    Returns dict: decision, walk, lists {frameID: {1, 2, 3}}, frames (in window order, for cloud())"""
    th = fref.median_hessian(post)
    dec = fref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=th)["decision"]
    w = walk(point_lists(win["host"], win["nf"]), dec)
    lists = lists_after(win, post, w)
    return dict(decision=dec, th=th, walk=w, lists=lists, frames=[dict(lists=lists[int(f)]) for f in win["frameID"]])
