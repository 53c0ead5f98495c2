"""FullSystem::removeOutliers + flagPointsForRemoval restated in numpy over (window, post-state arrays, frame_marg, last_gone, settings):
the reference of sdso_ba_flag_points, and the three windows its tests run on.

Reference: FullSystemOptimize.cpp:1063-1084 (removeOutliers), FullSystem.cpp:965-1056 (flagPointsForRemoval), HessianBlocks.h:439-469
(PointHessian::isOOB / isInlierNew), FullSystemOptimize.cpp:165-195 (linearizeAll(true): lastResiduals[k].second takes state_state
before the residuals on toRemove leave ph->residuals).  Written from those lines, array-wise — it shares no code with csrc/ba_flag.h."""
import numpy as np

import helpers
import synth

KEEP, DROP_NO_RESIDUAL, DROP_NEGATIVE, MARGINALIZE, DROP_WEAK, DROP_NOT_INLIER = range(6)
IN, OOB, OUTLIER = 0, 1, 2

#        nf, pts_per_kf, seed, flagged frames, codes 0..5 on the CPU oracle's post-state
CASES = {"A": dict(nf=8, pts_per_kf=40, seed=11, frame_marg=(0, 2), oracle_codes=(105, 51, 1, 81, 46, 36)),
         "B": dict(nf=5, pts_per_kf=120, seed=3001, frame_marg=(0,), oracle_codes=(197, 107, 0, 108, 44, 144)),
         "C": dict(nf=4, pts_per_kf=60, seed=7, frame_marg=(0,), oracle_codes=(59, 47, 0, 38, 8, 88))}


def make_case(name):
    """(window, frame_marg [nf] uint8, last_gone [2 np] uint8): a 640x480 window with a history of good residuals, residual lists that
    went through dropResidual's swap-with-last, and a caller history on a part of the lastResiduals slots."""
    c = CASES[name]
    win = synth.ba_window(w=640, h=480, nf=c["nf"], pts_per_kf=c["pts_per_kf"], seed=c["seed"])
    npts = win["np"]
    rs = np.random.RandomState(5)
    win = dict(win)
    win["numGoodResiduals"] = rs.randint(0, 20, npts).astype(np.int32)
    win, _ = helpers.drop_residuals(win, seed=11, drop_frac=0.25)
    last_gone = np.full(2 * npts, 255, np.uint8)
    last_gone[1::2][rs.rand(npts) < 0.3] = OUTLIER
    last_gone[0::2][rs.rand(npts) < 0.1] = OUTLIER
    frame_marg = np.zeros(c["nf"], np.uint8)
    frame_marg[list(c["frame_marg"])] = 1
    return win, frame_marg, last_gone


def median_hessian(post):
    """minIdepthH_marg of the tests: the synthetic Hessians are ~1e7, so the default of 50 would never produce DROP_WEAK"""
    h = post["idepth_hessian"]
    return float(np.median(h[h > 0]))


def flag_points(win, post, frame_marg, last_gone=None, minGoodActiveResForMarg=3, minGoodResForMarg=4, minIdepthH_marg=50.0):
    """post: idepth, idepth_hessian, numGoodResiduals [np]; state_state, toRemove [nr] (sdso_ba_get_post_state).  Returns a dict:
    decision [np] uint8, counts [6], host_counts [nf, 6] int32, and what the coverage conditions look at: n (residuals left), clause (the
    isOOB clause that returned true, 0 = isOOB false or not reached), host_only (leaves only because its host is flagged)."""
    nf, npts = win["nf"], win["np"]
    rp, rt = np.asarray(win["res_point"], np.int64), np.asarray(win["res_target"], np.int64)
    host = np.asarray(win["host"], np.int64)
    marg = np.asarray(frame_marg, np.uint8) != 0
    st = np.asarray(post["state_state"])
    alive = np.asarray(post["toRemove"]) == 0
    n = np.bincount(rp[alive], minlength=npts)                                        # ph->residuals.size() after :176-195
    vis = np.bincount(rp[alive & (st == IN) & marg[rt]], minlength=npts)              # HessianBlocks.h:442-448
    last = np.full((npts, 2), 255, np.int64)
    for k in range(2):
        sel = rt == nf - 1 - k                                                        # (a point observes a target at most once)
        last[rp[sel], k] = st[sel]                                                    # FullSystemOptimize.cpp:167-173, toRemove or not
    gone = np.full((npts, 2), 255, np.int64) if last_gone is None else np.asarray(last_gone, np.int64).reshape(npts, 2)
    last = np.where(gone != 255, gone, np.where(last != 255, last, OOB))
    good = np.asarray(post["numGoodResiduals"], np.int64)
    idepth, idh = np.asarray(post["idepth"], np.float32), np.asarray(post["idepth_hessian"], np.float32)
    c1 = (n >= minGoodActiveResForMarg) & (good > minGoodResForMarg + 10) & (n - vis < minGoodActiveResForMarg)
    c2 = ~c1 & (last[:, 0] == OOB)
    c3 = ~c1 & ~c2 & (n >= 2) & (last[:, 0] == OUTLIER) & (last[:, 1] == OUTLIER)
    oob = c1 | c2 | c3
    inlier = (n >= minGoodActiveResForMarg) & (good >= minGoodResForMarg)
    leaves = oob | marg[host]
    dec = np.full(npts, KEEP, np.uint8)
    dec[leaves & ~inlier] = DROP_NOT_INLIER
    dec[leaves & inlier] = DROP_WEAK
    dec[leaves & inlier & (idh > np.float32(minIdepthH_marg))] = MARGINALIZE
    dec[idepth < 0] = DROP_NEGATIVE
    dec[n == 0] = DROP_NO_RESIDUAL
    reached = (n > 0) & ~(idepth < 0)
    clause = np.where(reached, c1 * 1 + c2 * 2 + c3 * 3, 0)
    hc = np.zeros((nf, 6), np.int32)
    np.add.at(hc, (host, dec.astype(np.int64)), 1)
    return dict(decision=dec, counts=hc.sum(0).astype(np.int32), host_counts=hc, n=n, clause=clause, host_only=reached & ~oob & marg[host])


def check_coverage(name, r):
    """The conditions that keep a comparison on this case from being vacuous (asserted on the oracle's post-state and on the device's).
    Code 2 is counted over the cases together by the caller: returns its count."""
    cnt = r["counts"]
    for code in (KEEP, DROP_NO_RESIDUAL, MARGINALIZE, DROP_WEAK, DROP_NOT_INLIER):
        assert cnt[code] >= 5, (name, code, cnt)
    if name == "A":
        for cl in (1, 2, 3):
            assert (r["clause"] == cl).sum() >= 5, (cl, np.bincount(r["clause"], minlength=4))
        assert r["host_only"].sum() >= 1 and (r["n"] >= 7).sum() >= 1
    return int(cnt[DROP_NEGATIVE])
