"""Call time of sdso_ba_window_update (U) against hand-flatten + sdso_ba_upload_window (F) at configs[2] size, one process, alternating.

  F: numpy gather of every window array through the edit's maps (the cheapest flattening there is: the shim walks a pointer graph) +
     sdso_ba_upload_window + sdso_ctx_sync
  U: sdso_ba_window_update + sdso_ctx_sync
for two edits: the one after FullSystem::optimize (drop linearizeAll(true)'s toRemove, then the points left without a residual) and a full
keyframe edit (the oldest frame's points and the frame leave, 3 % of the points are dropped, a frame comes, the two newest hosts observe
it, 250 points are inserted with a residual into every other frame).  Host clock around the calls; before every repetition the window is
brought back to the state before the edit (fresh upload, and sdso_ba_marginalize_frame_dev for the keyframe edit), untimed.

  python tools/time_window_update.py [--reps 200] [--warmup 20] [--only-u]
--only-u is for a run under `rocprofv3 --kernel-trace --stats -- python tools/time_window_update.py --only-u`: the kernels alone."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi            # noqa: E402
import synth                        # noqa: E402
import window_edit_cases as cases   # noqa: E402
import window_edit_ref as ref       # noqa: E402
import window_update_helpers as wu  # noqa: E402

WID = 3


def keyframe_edit(win, rs):
    nf, npts = win["nf"], win["np"]
    marg = [int(p) for p in np.nonzero(win["host"] == 0)[0]]
    drop = ((rs.rand(npts) < 0.03) & (win["host"] != 0)).astype(np.uint8)
    stay = (win["host"] != 0) & (drop == 0)
    add_res = [(int(p), nf) for p in np.nonzero(stay & (win["host"] >= nf - 2))[0]]
    src = np.nonzero(win["host"] == 0)[0][:250]                  # the new frame is a copy of the one that leaves: its points serve as payload
    hosts = [nf] * len(src)
    pt_res = [(q, t) for q in range(len(src)) for t in range(1, nf)]
    edit = dict(remove_points=marg, drop_point=drop, remove_frames=[0], n_add_frames=1, add_res=add_res, add_points=hosts, pt_res=pt_res)
    payload = dict(add_frames={k: np.ascontiguousarray(np.asarray(win[k])[:1]) for k in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH")},
                   add_points={k: np.ascontiguousarray(win[k][src]) for k in ("u", "v", "idepth", "idepth_zero", "color", "weights", "hasDepthPrior")})
    payload["add_frames"]["frameID"] = np.array([900], np.int32)
    payload["add_frames"]["pyrs"] = [win["pyrs"][0]]
    return edit, payload


def gather_arrays(win, vals, maps, news):
    """what a caller copies to flatten the edited window: every per-frame / per-point / per-residual array through its map"""
    out = []
    for key, src in (("frame", maps[0]), ("point", maps[1]), ("res", maps[2])):
        idx = np.maximum(np.asarray(src), 0)
        for a in news[key]:
            out.append(np.ascontiguousarray(a[idx]))
    return out


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return "median %7.1f   p10 %7.1f   p90 %7.1f   min %7.1f  (us, n=%d)" % (np.median(t), t[len(t) // 10], t[(9 * len(t)) // 10], t[0], len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-u", action="store_true")
    args = ap.parse_args()
    ctx = abi.Context(0)
    win = synth.ba_window(w=1232, h=368, nf=8, pts_per_kf=250, seed=3001)
    wu.upload_pyramids(ctx, win)
    ctx.upload_pyramid(wu.SLOT0 + 900, win["pyrs"][0][:1])
    W0, keep0 = wu.make_window(win)
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, WID, C.byref(W0)))
    wu.optimize(ctx, WID)
    d = wu.post_state(ctx, WID, win)
    vals = wu.values_from_post(win, d)
    rs = np.random.RandomState(5)
    jobs = []
    for name, (edit, payload) in (("after optimize", (wu.outlier_edit(win, d), {})), ("keyframe", keyframe_edit(win, rs))):
        leaves = bool(edit.get("remove_frames"))
        n2 = 8 * (win["nf"] - (1 if leaves else 0) + edit.get("n_add_frames", 0)) + 4
        w2, maps = wu.flatten(win, vals, edit, payload, HM=np.zeros((n2, n2)), bM=np.zeros(n2))
        WF, keepF = wu.make_window(w2)
        pl = dict(payload)
        if "add_frames" in pl:
            pl["add_frames"] = dict(pl["add_frames"], frame_slot=[wu.SLOT0 + 900])
        E, keepE = cases.to_abi(edit, pl)
        news = dict(frame=[np.asarray(vals[k]) for k in ("evalPT", "state", "state_zero", "frameEnergyTH")] + [np.asarray(win[k]) for k in ("ab_exposure", "frameID")],
                    point=[np.asarray(win[k]) for k in ("u", "v", "color", "weights", "hasDepthPrior")] + [np.asarray(vals[k]) for k in ("idepth", "idepth_zero", "maxRelBaseline", "numGoodResiduals")],
                    res=[np.asarray(vals["res_state"])])
        jobs.append(dict(name=name, edit=edit, leaves=leaves, maps=maps, WF=WF, E=E, news=news, keep=(keepF, keepE), w2=w2,
                         tF_g=[], tF_c=[], tU=[]))
        print("%s: np %d -> %d, nr %d -> %d, nf %d -> %d" % (name, win["np"], w2["np"], win["nr"], w2["nr"], win["nf"], w2["nf"]))

    def reset(job):
        ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, WID, C.byref(W0)))
        if job["leaves"]:
            wu.marginalize_frame_dev(ctx, WID, 0, win["nf"] - 1)
        ctx.sync()

    for rep in range(args.warmup + args.reps):
        for job in jobs:
            if not args.only_u:
                reset(job)
                t0 = time.perf_counter()
                gather_arrays(win, vals, job["maps"], job["news"])
                t1 = time.perf_counter()
                ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, WID, C.byref(job["WF"])))
                ctx.sync()
                t2 = time.perf_counter()
                if rep >= args.warmup:
                    job["tF_g"].append(t1 - t0); job["tF_c"].append(t2 - t1)
            reset(job)
            t0 = time.perf_counter()
            rc = ctx.L.sdso_ba_window_update(ctx.h, WID, C.byref(job["E"]))
            ctx.sync()
            t1 = time.perf_counter()
            ctx.check(rc)
            if rep >= args.warmup:
                job["tU"].append(t1 - t0)
    for job in jobs:
        print(job["name"])
        if not args.only_u:
            print("  F gather (numpy)                      ", stats(job["tF_g"]))
            print("  F sdso_ba_upload_window + sync        ", stats(job["tF_c"]))
            print("  F total                               ", stats(np.asarray(job["tF_g"]) + np.asarray(job["tF_c"])))
        print("  U sdso_ba_window_update + sync        ", stats(job["tU"]))
    ctx.close()


if __name__ == "__main__":
    main()
