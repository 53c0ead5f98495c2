#!/usr/bin/env python3
"""sdso_g2o_lba_optimize — the fork-live window optimiser on the device — against the only route the library offered before it: a host
Levenberg-Marquardt over sdso_g2o_lba_eval that downloads error (nr x 8 doubles) and J (nr x 8 x 13 doubles) for every evaluation.

Window: 8 keyframes x --pts points each (250: 2000 points, about 14 000 residuals) at 1232 x 368, --iters iterations (the fork's count for a full window,
FullSystemOptimize.cpp:416-418).  The host route is tests/g2o_lba_ref.py with the device edge in place of the oracle: the same
algorithm, its linear algebra in NumPy.  The routes take turns in one process; medians of --reps calls after --warm warm-ups, every
timed window ending when the call returns.  For the host route the time spent inside sdso_g2o_lba_eval alone is reported too: the part
no host implementation can avoid.  Kernel times come from sdso_prof_read (HIP events) in a pass of their own.

  python tools/time_g2o_lba.py [--pts 250] [--iters 3] [--reps 50] [--warm 5] [--out profiles/g2o_lba_optimize_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi          # noqa: E402
import g2o_lba_ref as ref         # noqa: E402
import synth                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pts", type=int, default=250)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


W, H, NF = 1232, 368, 8
win = synth.ba_window(w=W, h=H, nf=NF, pts_per_kf=a.pts, seed=3001)
rp = win["res_point"]
rs = np.random.RandomState(3002)
c = dict(name="timing", nf=NF, nr=len(rp), w=W, h=H, win=win, iterations=a.iters, lambda_init=0.1,
         Ttw=[(np.array(p[0], np.float64), np.array(p[1], np.float64)) for p in win["poses"]],
         target_aff=[(float(x), float(y)) for x, y in win["affs"]], ab_exposure=win["ab_exposure"].copy(),
         host_b0=np.array([win["affs"][h][1] for h in range(NF)], np.float64), frameEnergyTH=win["frameEnergyTH"].copy(),
         host=np.ascontiguousarray(win["host"][rp], np.int32), target=np.ascontiguousarray(win["res_target"], np.int32),
         u=np.ascontiguousarray(win["u"][rp]), v=np.ascontiguousarray(win["v"][rp]),
         color=np.ascontiguousarray(win["color"][rp]), weights=np.ascontiguousarray(win["weights"][rp]),
         Twh=[synth.se3_mul(synth.se3_exp(rs.randn(6) * 5e-4), synth.se3_inv(win["poses"][h])) for h in range(NF)],
         host_aff=[(float(x), float(y)) for x, y in win["affs"]], cam=np.array([float(x) for x in win["K"]], np.float64),
         idepth=np.ascontiguousarray(win["idepth"][rp], np.float64))
nr = c["nr"]
ctx = abi.Context(0)
slots = [900 + f for f in range(NF)]
for f in range(NF):
    ctx.upload_pyramid(slots[f], win["pyrs"][f][:1])
slot_arr = np.ascontiguousarray(slots, np.int32)
eval_s = [0.0, 0]


def device_eval(_orc, c, Twh, aff, cam, idepth):
    """ref.oracle_eval's contract on sdso_g2o_lba_eval"""
    pR, pt, pab = ref.pair_tables(c, Twh, aff)
    S = abi.G2oLba()
    S.nf, S.nr, S.w, S.h = NF, nr, W, H
    S.cam[:] = [float(x) for x in cam]
    idp = np.ascontiguousarray(idepth, np.float64)
    S.frame_slot = abi.ip(slot_arr)
    S.pair_R, S.pair_t, S.pair_ab = abi.fp(pR), abi.fp(pt), abi.fp(pab)
    S.host_b0, S.frameEnergyTH = abi.dp(c["host_b0"]), abi.fp(c["frameEnergyTH"])
    S.host, S.target, S.u, S.v = abi.ip(c["host"]), abi.ip(c["target"]), abi.fp(c["u"]), abi.fp(c["v"])
    S.idepth, S.color, S.weights = abi.dp(idp), abi.fp(c["color"]), abi.fp(c["weights"])
    o = dict(error=np.empty((nr, 8)), J=np.empty((nr, 8, 13)), state=np.empty(nr, np.uint8), energy=np.empty((nr, 2), np.float32),
             cpt=np.empty((nr, 3), np.float32), ih=np.empty(nr, np.float32), lvl=np.empty(nr, np.uint8), tables=(pR, pt, pab))
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_g2o_lba_eval(ctx.h, C.byref(S), abi.dp(o["error"]), abi.dp(o["J"]), abi.bp(o["state"]), abi.fp(o["energy"]), abi.fp(o["cpt"]),
                                      abi.fp(o["ih"]), abi.bp(o["lvl"])))
    eval_s[0] += time.perf_counter() - t0
    eval_s[1] += 1
    return o


def route_host():
    eval_s[0], eval_s[1] = 0.0, 0
    t0 = time.perf_counter()
    r = ref.optimize(None, c, evaluate=device_eval)
    return time.perf_counter() - t0, eval_s[0], eval_s[1], r


def route_device():
    Wd, P, S, out, arr = ref.make_call(c, slots)
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_g2o_lba_optimize(ctx.h, C.byref(Wd), C.byref(P), C.byref(S), C.byref(out)))
    return time.perf_counter() - t0, out, S, arr


th, te, td = [], [], []
for k in range(a.warm + a.reps):
    h = route_host()
    d = route_device()
    if k >= a.warm:
        th.append(h[0]); te.append(h[1]); td.append(d[0])
r, out = h[3], d[1]
say("sdso_g2o_lba_optimize vs a host LM over sdso_g2o_lba_eval: %d keyframes, %d residuals, %d x %d, %d iterations" % (NF, nr, W, H, a.iters))
say("  both routes: iterations %d / %d, trials %s / %s, stop %d / %d, chi2 %.9g / %.9g" %
    (r["iterations"], out.iterations, r["trials"], list(out.trials[:out.iterations]), r["stop"], out.stop, r["chi2_final"], out.chi2_final))
say("  host LM over sdso_g2o_lba_eval   median %.2f ms (min %.2f) of %d; inside sdso_g2o_lba_eval: %.2f ms over %d evaluations, %.1f MB down each" %
    (1e3 * np.median(th), 1e3 * min(th), a.reps, 1e3 * np.median(te), h[2], nr * 8 * 14 * 8 / 1e6))
say("  sdso_g2o_lba_optimize            median %.2f ms (min %.2f) of %d" % (1e3 * np.median(td), 1e3 * min(td), a.reps))
say("  host route / device route = %.1f;  evaluations alone / device route = %.1f" % (np.median(th) / np.median(td), np.median(te) / np.median(td)))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 2))
ctx.check(ctx.L.sdso_prof_reset(ctx.h))
for _ in range(5):
    route_device()
tot = 0.0
for kname in ("k_lba_opt_eval", "k_lba_opt_lin", "k_lba_opt_schur"):
    ms, cnt = ctx.prof_read(kname)
    tot += ms / 5
    say("  kernel %-16s %.1f us x %d per call" % (kname, 1e3 * ms / max(cnt, 1), cnt // 5))
say("  kernels per call: %.3f ms (event brackets: they include the launch latency)" % tot)
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
