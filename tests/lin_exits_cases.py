"""One small BA window on which the linearisation (PointFrameResidual::linearize, Residuals.cpp:83-336) leaves through EVERY exit:
sticky OOB, `drescale <= 0`, centre out of bounds, pattern pixel out of bounds, and to the end (IN and OUTLIER).  The bit-exact
linearisation tests elsewhere run on windows without a single OOB residual (tests/test_ba_tiles_gpu.py asserts it).

`synth.ba_window(163, 98, nf=4, pts_per_kf=60, seed=3263)` — 240 points, 627 residuals, level 0 only — doctored by point index p and
residual index i:

    p % 8 == 1   idepth_zero = -40           the FEJ point behind the camera: drescale <= 0
    p % 8 == 3   idepth_zero *= 10           the FEJ centre thrown out of the image
    p % 8 == 5   idepth *= 10                the centre stays (idepth_zero untouched), pattern pixels leave
    i % 11 == 5  res_state = 1               OOB before the first linearisation: sticky

`classify_exits` names the exit of every residual that is not preset-sticky in float64 numpy, from the window's evalPT, K and idepths.
`oracle_rounds` runs linearize + applyRes twice on the CPU oracle: in the second round every OOB residual of the first is sticky.
"""
import ctypes as C

import numpy as np

from sdso_amd import abi
import synth

W, H, NF, PTS_PER_KF, SEED = 163, 98, 4, 60, 3263
EXITS = ("drescale", "centre", "pattern", "ran")


def window():
    win = synth.ba_window(W, H, nf=NF, pts_per_kf=PTS_PER_KF, seed=SEED)
    p = np.arange(win["np"])
    win["idepth_zero"] = win["idepth_zero"].copy()
    win["idepth"] = win["idepth"].copy()
    win["idepth_zero"][p % 8 == 1] = np.float32(-40.0)
    win["idepth_zero"][p % 8 == 3] *= np.float32(10.0)
    win["idepth"][p % 8 == 5] *= np.float32(10.0)
    win["res_state"] = win["res_state"].copy()
    win["res_state"][preset_sticky(win["nr"])] = 1
    return win


def preset_sticky(nr):
    return np.arange(nr) % 11 == 5


def classify_exits(win):
    """exit of every residual (index into EXITS; -1 for the preset-sticky ones), float64"""
    w, h, nf = win["w"], win["h"], win["nf"]
    idz, idp = win["idepth_zero"].astype(np.float64), win["idepth"].astype(np.float64)
    fx, fy, cx, cy = [float(x) for x in win["K"]]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    T = [(win["evalPT"][k][:9].reshape(3, 3), win["evalPT"][k][9:]) for k in range(nf)]
    inside = lambda a, b: a > 1.1 and b > 1.1 and a < w - 3 and b < h - 3
    sticky = preset_sticky(win["nr"])
    out = np.full(win["nr"], -1, np.int64)
    for i in range(win["nr"]):
        if sticky[i]:
            continue
        pt, t = win["res_point"][i], win["res_target"][i]
        R, tt = synth.se3_mul(T[t], synth.se3_inv(T[win["host"][pt]]))
        u, v = float(win["u"][pt]), float(win["v"][pt])
        P = R @ (Ki @ np.array([u, v, 1.0])) + tt * idz[pt]
        if not (P[2] != 0 and 1.0 / P[2] > 0):
            out[i] = 0
        elif not inside(P[0] / P[2] * fx + cx, P[1] / P[2] * fy + cy):
            out[i] = 1
        else:
            KRKi, Kt = K @ R @ Ki, K @ tt
            q = [KRKi @ np.array([u + dx, v + dy, 1.0]) + Kt * idp[pt] for dx, dy in synth.PATTERN]
            out[i] = 3 if all(inside(a[0] / a[2], a[1] / a[2]) for a in q) else 2
    return out


def _read(oracle, hd, nr):
    o = dict(Jn=np.zeros((nr, 74), np.float32), ns=np.zeros(nr, np.uint8), ne=np.zeros(nr, np.float32), nw=np.zeros(nr, np.float32),
             Je=np.zeros((nr, 74), np.float32), st=np.zeros(nr, np.uint8), act=np.zeros(nr, np.uint8), jp=np.zeros((nr, 8), np.float32))
    oracle.orc_ba_linearize(hd, None)
    oracle.orc_ba_get_linearization(hd, abi.fp(o["Jn"]), abi.bp(o["ns"]), abi.fp(o["ne"]), abi.fp(o["nw"]), None, None)
    oracle.orc_ba_apply_res(hd)
    oracle.orc_ba_get_ef_jacobians(hd, abi.fp(o["Je"]))
    oracle.orc_ba_get_residual_state(hd, abi.bp(o["st"]), abi.bp(o["act"]), abi.fp(o["jp"]))
    for a in o.values():
        a.setflags(write=False)
    return o


def oracle_rounds(oracle, win, new_frame_th=True):
    """[round 1, round 2] of linearize + applyRes on the oracle: ns, ne, nw, Jn as linearize left them, st, act, jp, Je after applyRes.
    new_frame_th: round 2 runs at the newest frame's threshold that round 1's setNewFrameEnergyTH left (FullSystem::linearizeAll,
    FullSystemOptimize.cpp:142-203) — the un-fused sdso_ba_linearize does the same.  False: at the uploaded thresholds, which is what
    sdso_ba_batch_accumulate does (linearize + applyRes + accumulate; the batch's setNewFrameEnergyTH belongs to its solve phase): the
    oracle's round 2 is then the first round of a window created with the states round 1 left."""
    def run(w, n):
        Wd, keep = abi.make_ba_window(w, dI_list=[p[0] for p in w["pyrs"]])
        hd = oracle.orc_ba_create(C.byref(Wd))
        try:
            return [_read(oracle, hd, w["nr"]) for _ in range(n)]
        finally:
            oracle.orc_ba_destroy(hd)
    if new_frame_th:
        return run(win, 2)
    o1 = run(win, 1)[0]
    win2 = dict(win)
    win2["res_state"] = o1["st"].copy()
    return [o1, run(win2, 1)[0]]
