"""Call time of the keyframe hand-over between the BA window and point activation, all-host route (F) against device-to-device route
(N), one process, the two routes taking turns.

  F map    : sdso_ba_get_state + the caller's flattening of u / v / host + sdso_distmap_make
  F insert : sdso_imm_activate_fetch + the stage-7 payload (NumPy, by the rules of include/sdso_abi.h) + sdso_ba_window_update + sdso_ctx_sync
  N map    : sdso_distmap_make_from_window (n_seeds = NULL) + sdso_ctx_sync
  N insert : sdso_ba_window_update_activated + sdso_ctx_sync
sdso_imm_activate itself is common to both routes and timed on its own.  Host clock around the calls; median of --reps repetitions after
--warmup.  Before every repetition the window is uploaded afresh and the groups are put again, untimed.  The shapes are the small ones of
tests/test_window_activated_gpu.py (640 x 480, four frames, 160 window points, 1 297 candidates); the seeds of the map are the window's own
points, as in tests/test_distmap_window_gpu.py's chain.  At the end the two routes' windows must agree in sdso_ba_get_state, bit for bit.

  python tools/time_activate_insert.py [--reps 50] [--warmup 5] [--out profiles/activated_insert_timing.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi                 # noqa: E402
import activate_cases as AC              # noqa: E402
import distmap_cases as DC               # noqa: E402
import pyoracle                          # noqa: E402
import synth                             # noqa: E402
import window_activated_helpers as wa    # noqa: E402
import window_update_helpers as wu       # noqa: E402

W, H = wa.W, wa.H
WN, WF = 13, 14
SLOT = 2340
IDS = {"F": [2400, 2401, 2402, 2403], "N": [2410, 2411, 2412, 2413]}
ACT_FRAME = [0, 1, 2, 3]


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return "median %8.1f   p10 %8.1f   p90 %8.1f   min %8.1f  (us, n=%d)" % (np.median(t), t[len(t) // 10], t[(9 * len(t)) // 10], t[0], len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activated_insert_timing.txt"))
    args = ap.parse_args()
    orc = pyoracle.load()
    ctx = abi.Context(0)
    base = wu.with_history(synth.ba_window(w=W, h=H, nf=4, pts_per_kf=40, seed=4101), 31)
    c0 = AC.window(orc)
    win = c0["win"]
    slots = [SLOT + f for f in range(4)]
    for f in range(4):
        ctx.upload_pyramid(slots[f], [win["imgs"][f]])
    wu.upload_pyramids(ctx, base)
    W0, keep0 = wu.make_window(base)
    KRKi4 = np.concatenate([win["KRKi"], win["KRKi"][:1]])          # a geometry per window frame; the newest is skipped
    Kt4 = np.concatenate([win["Kt"], win["Kt"][:1]])
    G4 = abi.make_distmap_geoms(KRKi4, Kt4)
    skip = np.array([0, 0, 0, 1], np.uint8)
    empty_edit, keep_e = wa.edit_abi({})
    act_frame = np.array(ACT_FRAME, np.int32)
    n_cand = sum(len(S["u"]) for S in win["groups"][:3])
    t = {k: [] for k in ("F map", "F insert", "N map", "N insert", "F activate", "N activate")}
    L = ctx.L

    def reset(route, wid):
        wa.release_groups(ctx, IDS[route])
        ctx.check(L.sdso_ba_upload_window(ctx.h, wid, C.byref(W0)))
        wa.put_groups(ctx, IDS[route], AC.window(orc)["win"]["groups"])
        ctx.sync()

    def activate(route):
        rc, counts = ctx.imm_activate_raw(min_obs=1, min_act_dist=float(c0["min_act_dist"]), **wa.activate_args(win, IDS[route], slots))
        ctx.check(rc)
        return counts

    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        # ---- route F
        reset("F", WF)
        t0 = time.perf_counter()
        idp = np.zeros(base["np"], np.float32)
        ctx.check(L.sdso_ba_get_state(ctx.h, WF, None, abi.fp(idp), None))
        sel = base["host"] < 3
        n_f = DC.dm_make(ctx, W, H, KRKi4, Kt4, base["host"][sel], base["u"][sel], base["v"][sel], idp[sel])
        t1 = time.perf_counter()
        counts_f = activate("F")
        t2 = time.perf_counter()
        rec = ctx.imm_activate_fetch(n_cand, int(counts_f[4]), 4)
        e7, p7, idx = wa.stage7(rec, ACT_FRAME)
        rc = wu.update(ctx, WF, e7, p7)
        ctx.sync()
        t3 = time.perf_counter()
        ctx.check(rc)
        # ---- route N
        reset("N", WN)
        u0 = time.perf_counter()
        ctx.check(L.sdso_distmap_make_from_window(ctx.h, WN, W, H, G4, abi.bp(skip), None))
        ctx.sync()
        u1 = time.perf_counter()
        counts_n = activate("N")
        u2 = time.perf_counter()
        n_pt, n_res = C.c_int(-1), C.c_int(-1)
        act_index = np.full(max(1, int(counts_n[4])), -1, np.int32)
        rc = L.sdso_ba_window_update_activated(ctx.h, WN, C.byref(empty_edit), abi.ip(act_frame), C.byref(n_pt), C.byref(n_res), abi.ip(act_index))
        ctx.sync()
        u3 = time.perf_counter()
        ctx.check(rc)
        if keep:
            for k, v in (("F map", t1 - t0), ("F activate", t2 - t1), ("F insert", t3 - t2), ("N map", u1 - u0), ("N activate", u2 - u1), ("N insert", u3 - u2)):
                t[k].append(v)
    # ---- the two windows agree
    assert np.array_equal(counts_f, counts_n) and n_pt.value == len(idx) and np.array_equal(act_index[:n_pt.value], idx)
    s, _ = wa.sizes_after(base, e7)
    st = {}
    for wid in (WF, WN):
        a = (np.zeros((s["nf"], 10)), np.zeros(s["np"], np.float32), np.zeros(s["nr"], np.uint8))
        ctx.check(L.sdso_ba_get_state(ctx.h, wid, abi.dp(a[0]), abi.fp(a[1]), abi.bp(a[2])))
        st[wid] = a
    same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(st[WF], st[WN]))
    lines = ["keyframe hand-over, route F (all host) against route N (device to device): 640 x 480, nf 4, window %d points / %d residuals," % (base["np"], base["nr"]),
             "%d candidates, toOptimize %d, %d points with %d residuals appended; window afterwards %d points / %d residuals" %
             (n_cand, int(counts_n[4]), n_pt.value, n_res.value, s["np"], s["nr"]),
             "sdso_ba_get_state of the two windows agrees bit for bit: %s" % same, ""]
    for k in ("F map", "N map", "F activate", "N activate", "F insert", "N insert"):
        lines.append("  %-12s %s" % (k, stats(t[k])))
    lines.append("  %-12s %s" % ("F map+insert", stats(np.asarray(t["F map"]) + np.asarray(t["F insert"]))))
    lines.append("  %-12s %s" % ("N map+insert", stats(np.asarray(t["N map"]) + np.asarray(t["N insert"]))))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)
    ctx.close()
    assert same, "the two routes' windows differ"


if __name__ == "__main__":
    main()
