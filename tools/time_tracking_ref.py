"""Times CoarseTracker::setCoarseTrackingRef -> makeCoarseDepthL0 after FullSystem::optimize two ways in one process, at the benchmark
window (8 keyframes x 250 points, 1232x368) and at 7 x 570 points:
  (a) the route over the host: sdso_ba_get_post_state with the projections, STEP1's gather on the host, sdso_stereo_match_batch, the accept
      rule, sdso_track_make_ref
  (b) sdso_track_make_ref_from_window with pc_n_out requested
Median of --reps calls of each route after --warm warm-ups, the two routes taking turns; every timed window ends when the call returns
(both leave the template's counts on the host).  The templates of the two routes are compared bit for bit.  Kernel times come from
sdso_prof_read in a pass of their own (profiling level 2 puts two event records around every launch).
  python tools/time_tracking_ref.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/tracking_ref_resident_ab.txt is such a report)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import tracking_ref_window_cases as TC

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
SHAPES = (("8 KF x 250 points", dict(w=1232, h=368, nf=8, pts_per_kf=250, seed=3001)), ("7 KF x 570 points", dict(w=1232, h=368, nf=7, pts_per_kf=570, seed=3002)))
KERNELS = ("k_ref_gather", "k_ref_accept", "k_trace_stereo")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


ctx = abi.Context(0)
say("setCoarseTrackingRef after optimize: host route (a) vs sdso_track_make_ref_from_window (b); %d calls each after %d warm-ups, 1232x368" % (REPS, WARM))
for si, (name, spec) in enumerate(SHAPES):
    case = TC.make_case(idepth_noise=0.05, drop_frac=0.1, **spec)
    up = TC.upload(ctx, case, 10 + si, 100 + 20 * si)
    TC.optimize(ctx, up["wid"], 3)

    split = []

    def route_a():
        clock = [time.perf_counter()]
        out = TC.host_route(ctx, case, up, 1, clock=clock)
        split.append(np.diff(clock))
        return out

    def route_b():
        rc, n, nb, pcn = TC.window_call(ctx, up, 2)
        ctx.check(rc)
        return n, pcn

    ta, tb = [], []
    for i in range(WARM + REPS):
        ctx.sync(); t0 = time.perf_counter(); ga, pcn_a = route_a(); t1 = time.perf_counter()
        ctx.sync(); t2 = time.perf_counter(); nb_, pcn_b = route_b(); t3 = time.perf_counter()
        if i >= WARM:
            ta.append(t1 - t0); tb.append(t3 - t2)
    la, lb = TC.get_ref(ctx, 1, case["levels"]), TC.get_ref(ctx, 2, case["levels"])
    same = all(np.array_equal(TC.bits(x[k]), TC.bits(y[k])) for x, y in zip(la, lb) for k in TC.KEYS) and np.array_equal(pcn_a, pcn_b)
    ma, mb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
    say()
    say("%s: np %d nr %d, %d points splatted, pc_n %s, templates identical: %s" % (name, case["np"], case["nr"], nb_, list(pcn_b[:case["levels"]]), same))
    say("  (a) host route   median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
    say("      of which (medians): post-state %.3f, gather in numpy %.3f, sdso_stereo_match_batch %.3f, accept rule in numpy %.3f, sdso_track_make_ref %.3f ms"
        % tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0)))
    say("  (b) from window  median %.3f ms   (min %.3f)" % (mb, 1e3 * min(tb)))
    say("  (a) / (b) = %.2f" % (ma / mb))
    # ---- kernel times, a pass of their own
    ctx.check(ctx.L.sdso_prof_enable(ctx.h, 2))
    for label, fn in (("a", route_a), ("b", route_b)):
        ctx.check(ctx.L.sdso_prof_reset(ctx.h))
        for _ in range(10):
            fn()
        ctx.sync()
        parts = []
        for k in KERNELS:
            ms, n = ctx.prof_read(k)
            if n:
                parts.append("%s %.1f us x %d" % (k, 1e3 * ms / n, n // 10))
        say("  kernels (%s), per launch x launches per call: %s" % (label, ", ".join(parts)))
    ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
    if not same:
        say("MISMATCH between the two routes")
        sys.exit(1)
ctx.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
