#!/usr/bin/env python3
"""sdso_g2o_lba_optimize_resident — the fork-live window optimiser with its Levenberg-Marquardt loop resident on the device — against
sdso_g2o_lba_optimize, the same optimiser with the loop's controller on the host (a launch and a wait per evaluation).

Workload (a): the window of tools/time_g2o_lba.py — 8 keyframes x --pts points each (250: about 13 000 residuals) at 1232 x 368, 3 iterations.
Workload (b): a 2-keyframe window with max_iterations = 10, the shape where the resident route's fixed schedule is longest against the
work it holds.
The routes take turns in one process; medians of --reps calls after --warm warm-ups (the method of tools/time_g2o_lba.py), every timed
window ending when the call returns.  For the resident route also: the host time of _enqueue alone (the fetch follows outside the
window), the kernels' times from sdso_prof_read (HIP events tied to each dispatch) in a pass of their own, and the launches that did work
against those that returned early.  The fixed schedule is known at enqueue and the controller is deterministic, so the two counts follow
from (max_iterations, max_trials) and the iterations / trials the call reports; a window without an active edge, whose launches all
return early after the first two, prices the early return: per kernel from its events, and as wall time per launch from the whole call
with and without the schedule.

  python tools/time_g2o_lba_resident.py [--pts 250] [--reps 50] [--warm 5] [--out profiles/g2o_lba_resident_timing.txt]
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []
W, H = 1232, 368
KERNELS = ("k_lbar_eval", "k_lbar_lin", "k_lbar_schur", "k_lbar_ctl")


def say(s):
    print(s, flush=True)
    lines.append(s)


def make_case(nf, seed, iters):
    win = synth.ba_window(w=W, h=H, nf=nf, pts_per_kf=a.pts, seed=seed)
    rp = win["res_point"]
    rs = np.random.RandomState(seed + 1)
    return dict(name="timing", nf=nf, nr=len(rp), w=W, h=H, win=win, iterations=iters, lambda_init=0.1,
                Ttw=[(np.array(p[0], np.float64), np.array(p[1], np.float64)) for p in win["poses"]],
                target_aff=[(float(x), float(y)) for x, y in win["affs"]], ab_exposure=win["ab_exposure"].copy(),
                host_b0=np.array([win["affs"][h][1] for h in range(nf)], np.float64), frameEnergyTH=win["frameEnergyTH"].copy(),
                host=np.ascontiguousarray(win["host"][rp], np.int32), target=np.ascontiguousarray(win["res_target"], np.int32),
                u=np.ascontiguousarray(win["u"][rp]), v=np.ascontiguousarray(win["v"][rp]),
                color=np.ascontiguousarray(win["color"][rp]), weights=np.ascontiguousarray(win["weights"][rp]),
                Twh=[synth.se3_mul(synth.se3_exp(rs.randn(6) * 5e-4), synth.se3_inv(win["poses"][h])) for h in range(nf)],
                host_aff=[(float(x), float(y)) for x, y in win["affs"]], cam=np.array([float(x) for x in win["K"]], np.float64),
                idepth=np.ascontiguousarray(win["idepth"][rp], np.float64))


ctx = abi.Context(0)
L, h = ctx.L, ctx.h


def route(fn, c, slots, **kw):
    Wd, P, S, out, arr = ref.make_call(c, slots, **kw)
    t0 = time.perf_counter()
    ctx.check(getattr(L, fn)(h, C.byref(Wd), C.byref(P), C.byref(S), C.byref(out)))
    return time.perf_counter() - t0, out, S, arr


def route_split(c, slots, **kw):
    Wd, P, S, out, arr = ref.make_call(c, slots, **kw)
    t0 = time.perf_counter()
    ctx.check(L.sdso_g2o_lba_optimize_enqueue(h, C.byref(Wd), C.byref(P), C.byref(S)))
    t1 = time.perf_counter()
    ctx.check(L.sdso_g2o_lba_optimize_fetch(h, C.byref(S), C.byref(out)))
    return t1 - t0, time.perf_counter() - t0


def counts(out, max_it, max_tr):
    """per kernel: (launches that did work, launches enqueued)"""
    tr = list(out.trials[:out.iterations])
    it = out.iterations
    return {"k_lbar_eval": (1 + sum(tr) + it, 1 + max_it * (max_tr + 1)), "k_lbar_lin": (it, max_it), "k_lbar_schur": (sum(tr), max_it * max_tr),
            "k_lbar_ctl": (1 + 2 * sum(tr) + it, 1 + max_it * (2 * max_tr + 1))}


def prof_pass(c, slots, n=5, **kw):
    ctx.check(L.sdso_prof_enable(h, 2))
    ctx.check(L.sdso_prof_reset(h))
    for _ in range(n):
        route("sdso_g2o_lba_optimize_resident", c, slots, **kw)
    res = {k: ctx.prof_read(k) for k in KERNELS}
    ctx.check(L.sdso_prof_enable(h, 0))
    ctx.check(L.sdso_prof_reset(h))
    return {k: (ms / n, cnt // n) for k, (ms, cnt) in res.items()}


def workload(tag, c, slots, max_it):
    nf, nr = c["nf"], c["nr"]
    for f in range(nf):
        ctx.upload_pyramid(slots[f], c["win"]["pyrs"][f][:1])
    th, tr_, te, ts = [], [], [], []
    for k in range(a.warm + a.reps):
        d = route("sdso_g2o_lba_optimize", c, slots)
        r = route("sdso_g2o_lba_optimize_resident", c, slots)
        s = route_split(c, slots)
        if k >= a.warm:
            th.append(d[0]); tr_.append(r[0]); te.append(s[0]); ts.append(s[1])
    o1, o2 = d[1], r[1]
    say("workload (%s): %d keyframes, %d residuals, %d x %d, max_iterations %d" % (tag, nf, nr, W, H, max_it))
    say("  both routes: iterations %d / %d, trials %s / %s, stop %d / %d, chi2 %.12g / %.12g" %
        (o1.iterations, o2.iterations, list(o1.trials[:o1.iterations]), list(o2.trials[:o2.iterations]), o1.stop, o2.stop, o1.chi2_final, o2.chi2_final))
    say("  sdso_g2o_lba_optimize (host-driven)    median %.3f ms (min %.3f) of %d" % (1e3 * np.median(th), 1e3 * min(th), a.reps))
    say("  sdso_g2o_lba_optimize_resident         median %.3f ms (min %.3f) of %d" % (1e3 * np.median(tr_), 1e3 * min(tr_), a.reps))
    say("  _enqueue alone (host time)             median %.3f ms (min %.3f); _enqueue + _fetch median %.3f ms" % (1e3 * np.median(te), 1e3 * min(te), 1e3 * np.median(ts)))
    say("  host-driven / resident = %.2f" % (np.median(th) / np.median(tr_)))
    # a window of the same shape without an active edge: every launch after the first two returns early
    e = dict(c)
    e["u"] = np.full_like(c["u"], -2000.0)
    t_sched = np.median([route("sdso_g2o_lba_optimize_resident", e, slots)[0] for _ in range(a.warm + 20)][a.warm:])
    t_none = np.median([route("sdso_g2o_lba_optimize_resident", e, slots, max_iterations=0)[0] for _ in range(a.warm + 20)][a.warm:])
    cn = counts(o2, max_it, 10)
    n_sched = sum(v[1] for v in cn.values()) - 2
    say("  an early-returning launch: %.2f us of wall time each (a window without an active edge: %.3f ms with its %d launches that return early, %.3f ms with max_iterations 0)" %
        (1e6 * (t_sched - t_none) / n_sched, 1e3 * t_sched, n_sched, 1e3 * t_none))
    early, early0, full = prof_pass(e, slots), prof_pass(e, slots, max_iterations=0), prof_pass(c, slots)
    tot = 0.0
    for k in KERNELS:
        worked, launched = cn[k]
        ms, cnt = full[k]
        assert cnt == launched, (k, cnt, launched)
        # the early return's price: the window without an active edge, its launches past those max_iterations 0 has too (which do work)
        e_us = 1e3 * (early[k][0] - early0[k][0]) / (early[k][1] - early0[k][1])
        w_us = (1e3 * ms - e_us * (launched - worked)) / max(worked, 1)
        tot += ms
        say("  kernel %-13s %4d launches, %3d did work, %4d returned early: %.3f ms in all; an early return %.2f us, a launch that did work %.1f us" %
            (k, launched, worked, launched - worked, ms, e_us, w_us))
    say("  kernels per call: %.3f ms (events tied to each dispatch)" % tot)
    return np.median(th), np.median(tr_)


ca = make_case(8, 3001, 3)
ha, ra = workload("a", ca, [900 + f for f in range(8)], 3)
cb = make_case(2, 3011, 10)
hb, rb = workload("b", cb, [920 + f for f in range(2)], 10)
say("resident below host-driven at (a): %s (%.3f ms against %.3f ms); at (b): %s (%.3f ms against %.3f ms)" %
    ("yes" if ra < ha else "NO", 1e3 * ra, 1e3 * ha, "yes" if rb < hb else "NO", 1e3 * rb, 1e3 * hb))
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
