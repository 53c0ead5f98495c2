"""Times FullSystem::removeOutliers + flagPointsForRemoval after FullSystem::optimize two ways in one process, at the benchmark window
(8 keyframes x 250 points, 1232x368):
  (a) the route over the host: sdso_ba_get_post_state with the seven per-point arrays, the residual states and toRemove, then the decision
      loop on the host (tests/flag_points_ref.py, numpy)
  (b) sdso_ba_flag_points
Median of --reps calls of each route after --warm warm-ups, the two routes taking turns; every timed window ends when the call returns.
The decisions of the two routes are compared byte for byte.  The kernel time comes from sdso_prof_read in a pass of its own.
  python tools/time_flag_points.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/flag_points_timing.txt is such a report).  There is no pass mark: the
result is a latency to report."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import flag_points_ref as ref
import helpers
import synth
import window_update_helpers as wu

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
WID = 12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def device_name():
    try:
        import torch
        name = torch.cuda.get_device_name(0)
        arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
        return ("%s (%s)" % (name, arch)) if name else (arch or "one MI355X (gfx950)")
    except Exception:
        return "one MI355X (gfx950)"      # the library is built for gfx950 only; the runtime gave no name


win = synth.ba_window(w=1232, h=368, nf=8, pts_per_kf=250, seed=3001)            # configs[2] of bench.py
rs = np.random.RandomState(5)
win = dict(win)
win["numGoodResiduals"] = rs.randint(0, 20, win["np"]).astype(np.int32)
win, _ = helpers.drop_residuals(win, seed=11, drop_frac=0.25)
nf, npts, nr = win["nf"], win["np"], win["nr"]
last_gone = np.full(2 * npts, 255, np.uint8)
last_gone[1::2][rs.rand(npts) < 0.3] = ref.OUTLIER
frame_marg = np.zeros(nf, np.uint8); frame_marg[[0, 2]] = 1

ctx = abi.Context(0)
wu.upload_pyramids(ctx, win)
keep = wu.upload(ctx, win, WID)
wu.optimize(ctx, WID)
th = ref.median_hessian(wu.post_state(ctx, WID, win))

# (a): only what the decision reads is asked for
post = dict(idepth=np.zeros(npts, np.float32), step=np.zeros(npts, np.float32), HdiF=np.zeros(npts, np.float32), bdSumF=np.zeros(npts, np.float32),
            idepth_hessian=np.zeros(npts, np.float32), maxRelBaseline=np.zeros(npts, np.float32), numGoodResiduals=np.zeros(npts, np.int32),
            state_state=np.zeros(nr, np.uint8), toRemove=np.zeros(nr, np.uint8))
P = abi.BAPostState()
abi.bind(P, post)
split = []


def route_a():
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_ba_get_post_state(ctx.h, WID, C.byref(P)))
    t1 = time.perf_counter()
    r = ref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=th)
    split.append((t1 - t0, time.perf_counter() - t1))
    return r["decision"], r["counts"], r["host_counts"]


F, keepF = abi.make_flag_points(frame_marg, last_gone, minIdepthH_marg=th)
dec, cnt, hc = np.zeros(npts, np.uint8), np.zeros(6, np.int32), np.zeros((nf, 6), np.int32)


def route_b():
    ctx.check(ctx.L.sdso_ba_flag_points(ctx.h, WID, C.byref(F), abi.bp(dec), abi.ip(cnt), abi.ip(hc)))
    return dec, cnt, hc


ta, tb = [], []
for i in range(WARM + REPS):
    ctx.sync(); t0 = time.perf_counter(); ra = route_a(); t1 = time.perf_counter()
    ctx.sync(); t2 = time.perf_counter(); rb = route_b(); t3 = time.perf_counter()
    if i >= WARM:
        ta.append(t1 - t0); tb.append(t3 - t2)
same = all(np.array_equal(x, y) for x, y in zip(ra, rb))
ma, mb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
say("removeOutliers + flagPointsForRemoval after optimize: host route (a) vs sdso_ba_flag_points (b) on %s" % device_name())
say("%d calls each after %d warm-ups, the routes taking turns; 8 KF x 250 points, 1232x368: np %d nr %d" % (REPS, WARM, npts, nr))
say("codes 0..5: %s, decisions identical: %s" % (rb[1].tolist(), same))
say("  (a) host route          median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
say("      of which (medians): sdso_ba_get_post_state %.3f, decision loop in numpy %.3f ms" % tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0)))
say("  (b) sdso_ba_flag_points median %.3f ms   (min %.3f)" % (mb, 1e3 * min(tb)))
say("  (a) / (b) = %.2f" % (ma / mb))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 2))
ctx.check(ctx.L.sdso_prof_reset(ctx.h))
for _ in range(10):
    route_b()
ctx.sync()
ms, n = ctx.prof_read("k_ba_flag_points")
say("  kernel (b): k_ba_flag_points %.1f us x %d per call" % (1e3 * ms / max(n, 1), n // 10))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
ctx.check(ctx.L.sdso_ba_release_window(ctx.h, WID))
ctx.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not same:
    print("MISMATCH between the two routes")
    sys.exit(1)
