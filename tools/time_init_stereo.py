"""Times the start of a sequence — CoarseInitializer::setFirstStereo, level 0 (CoarseInitializer.cpp:842-972) and STEP 3 of
FullSystem::initializeFromInitializer (FullSystem.cpp:1533-1573) — two ways in one process, at 1232x368:
  (a) composed from the older entry points: sdso_pixel_select with the map download, sdso_immature_init_batch, sdso_trace_stereo_batch, and
      the two rules (which pixels become Pnts, which Pnts become points) in NumPy
  (b) sdso_init_set_first_stereo + sdso_init_from_initializer + sdso_init_get_points
Median of --reps calls of each route after --warm warm-ups, the routes taking turns; every timed window ends when the call returns.  Both
routes use the same keep flags (a seeded generator at 2000 / numPoints), and their points are compared byte for byte.  The kernel times
come from sdso_prof_read in a pass of its own.
  python tools/time_init_stereo.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/init_first_stereo_timing.txt is such a report).  There is no pass mark: the
call runs once per sequence, so the result is an indication."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import init_cases as IC
import init_ref as IR

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 30, int), arg("--warm", 3, int), arg("--out", None, str)
W, H = 1232, 368
SLOT_L, SLOT_R = 1, 2
f32 = np.float32
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


P = IC.stereo_pair(W, H)
K4, baseline, density = P["K4"], P["baseline"], IC.density(W, H)
ctx = abi.Context(0)
L = ctx.L
ctx.upload_pyramid(SLOT_L, P["pyr_left"]); ctx.upload_pyramid(SLOT_R, [P["right"]])
n0, _ = ctx.init_set_first_stereo(SLOT_L, SLOT_R, K4, baseline)
keep = IC.keep_flags(n0, 5, IC.DESIRED_POINT_DENSITY / n0)
split = []


def route_a():
    t0 = time.perf_counter()
    m = np.zeros((H, W), f32)
    pot, num = C.c_int(3), C.c_int(0)
    ctx.check(L.sdso_pixel_select(ctx.h, SLOT_L, density, 1, 2.0, C.byref(pot), abi.fp(m), C.byref(num)))
    t1 = time.perf_counter()
    stamps = []

    def trace(u, v):
        n = len(u)
        col, wgt, gH, eth = [np.zeros(s, f32) for s in ((n, 8), (n, 8), (n, 4), (n,))]
        ctx.check(L.sdso_immature_init_batch(ctx.h, SLOT_L, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
        stamps.append(time.perf_counter())
        T, d = abi.make_trace_points(n, u, v, col, wgt, gH, eth)
        st = np.zeros(n, np.uint8)
        ctx.check(L.sdso_trace_stereo_batch(ctx.h, SLOT_R, abi.fp(K4), baseline, 1, C.byref(T), abi.bp(st)))
        stamps.append(time.perf_counter())
        return dict(status=st, energyTH=eth, idepth_min=d["idepth_min_stereo"], idepth_max=d["idepth_max_stereo"], idepth_stereo=d["idepth_stereo"], color=col,
                    weights=wgt)
    S = IR.set_first_with(m, trace)
    F = IR.from_initializer(S, keep)
    t2 = time.perf_counter()
    split.append((t1 - t0, stamps[0] - t1, stamps[1] - stamps[0], (t2 - stamps[1])))
    return S["n"], F["points"]


def route_b():
    n, _ = ctx.init_set_first_stereo(SLOT_L, SLOT_R, K4, baseline)
    npts, _ = ctx.init_from_initializer(keep)
    return n, ctx.init_get_points(npts)


ta, tb = [], []
for i in range(WARM + REPS):
    ctx.sync(); t0 = time.perf_counter(); na, ra = route_a(); t1 = time.perf_counter()
    ctx.sync(); t2 = time.perf_counter(); nb, rb = route_b(); t3 = time.perf_counter()
    if i >= WARM:
        ta.append(t1 - t0); tb.append(t3 - t2)
same = na == nb and all(np.ascontiguousarray(ra[k]).tobytes() == np.ascontiguousarray(rb[k]).tobytes() for k in IR.POINT)
ma, mb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
say("the stereo start of a sequence: composed from the older entry points (a) vs sdso_init_* (b) on %s" % device_name())
say("%d calls each after %d warm-ups, the routes taking turns; %dx%d, density %g: %d Pnts, %d points at keep = %g / numPoints; points identical: %s"
    % (REPS, WARM, W, H, density, nb, len(rb["pnt"]), IC.DESIRED_POINT_DENSITY, same))
say("  (a) older entry points + NumPy   median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
say("      of which (medians): sdso_pixel_select with its map %.3f, candidates and sdso_immature_init_batch %.3f, sdso_trace_stereo_batch %.3f, rules %.3f ms"
    % tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0)))
say("  (b) sdso_init_set_first_stereo + _from_initializer + _get_points   median %.3f ms   (min %.3f)   (a) / (b) = %.2f" % (mb, 1e3 * min(tb), ma / mb))
ctx.check(L.sdso_prof_enable(ctx.h, 2))
ctx.check(L.sdso_prof_reset(ctx.h))
for _ in range(10):
    route_b()
ctx.sync()
for k in ("k_init_map_count", "k_init_cand_count", "k_init_cand_write", "k_immature_init", "k_trace_stereo", "k_init_pnts", "k_init_select", "k_init_point_count",
          "k_init_point_write"):
    ms, cnt = ctx.prof_read(k)
    say("  kernel (b): %-20s %.1f us x %d per call" % (k, 1e3 * ms / max(cnt, 1), cnt // 10))
ctx.check(L.sdso_prof_enable(ctx.h, 0))
ctx.check(L.sdso_init_release(ctx.h))
ctx.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not same:
    print("MISMATCH between the routes")
    sys.exit(1)
