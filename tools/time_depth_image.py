"""Times the keyframe's depth image (CoarseTracker::debugPlotIDepthMap + debugPlotIDepthMapFloat, CoarseTracker.cpp:1071-1188) two ways
in one process, on a 1232x368 template of about 4000 points:
  (a) the route over the host: the w*h-float level-0 map copied to the host (hipMemcpy from the kept map), then tools/depth_image_cpu.cpp,
      a C++ -O3 single-thread restatement of :1071-1176 (std::sort, three passes over the image, one 40-pixel ring per depth pixel)
  (b) sdso_track_depth_image with both images asked for
Median of --reps calls of each route after --warm warm-ups, the two routes taking turns; every timed window ends when the call returns.
The images, the range and the counts of the two routes are compared byte for byte.  The kernel times come from sdso_prof_read in a pass
of their own.
  python tools/time_depth_image.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/depth_image_timing.txt is such a report).  There is no pass mark: the
result is a latency to report."""
import ctypes as C
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import synth

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
W, H, NPTS, FRAME, REF = 1232, 368, 4000, 5, 5
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


# the yardstick, built here
tmp = tempfile.mkdtemp(prefix="depth_image_cpu_")
lib = os.path.join(tmp, "libdepth_image_cpu.so")
subprocess.check_call([os.environ.get("CXX") or shutil.which("g++") or "g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                       os.path.join(ROOT, "tools", "depth_image_cpu.cpp"), "-o", lib])
cpu = C.CDLL(lib)
cpu.depth_image_cpu.argtypes = [abi.c_float_p, abi.c_float_p, C.c_int, C.c_int, abi.c_float_p, abi.c_float_p, abi.c_u8_p, abi.c_int_p]

prob = synth.tracker_problem(w=W, h=H, npts=NPTS, seed=2201)
u, v, idp = prob["points"]
wgt = np.random.RandomState(3).uniform(0.1, 30.0, NPTS).astype(np.float32)
dI0 = np.ascontiguousarray(prob["pyr_ref"][0], np.float32)

ctx = abi.Context(0)
ctx.keep_depth_map(True)
ctx.upload_pyramid(FRAME, prob["pyr_ref"])
pcn = np.zeros(8, np.int32)
ui, vi, idp = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32), np.ascontiguousarray(idp, np.float32)
ctx.check(ctx.L.sdso_track_make_ref(ctx.h, REF, FRAME, NPTS, abi.ip(ui), abi.ip(vi), abi.fp(idp), abi.fp(wgt), abi.ip(pcn)))
ctx.depth_image(REF, FRAME, W, H, (-1, -1))
p_rgb, p_map, _, _ = ctx.depth_image_dev(REF)

a_map, a_rgb, a_cnt = np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8), np.zeros(2, np.int32)
b_map, b_rgb, b_cnt = np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8), np.zeros(2, np.int32)
split = []


def route_a(rng):
    t0 = time.perf_counter()
    rc = ctx.L.hipMemcpy(C.c_void_p(a_map.ctypes.data), C.c_void_p(p_map), C.c_size_t(a_map.nbytes), 2)      # hipMemcpyDeviceToHost
    t1 = time.perf_counter()
    rc |= cpu.depth_image_cpu(abi.fp(a_map), abi.fp(dI0), W, H, abi.fp(rng[0:1]), abi.fp(rng[1:2]), abi.bp(a_rgb), abi.ip(a_cnt))
    split.append((t1 - t0, time.perf_counter() - t1))
    assert rc == 0


def route_b(rng):
    ctx.check(ctx.L.sdso_track_depth_image(ctx.h, REF, FRAME, abi.fp(rng[0:1]), abi.fp(rng[1:2]), abi.bp(b_rgb), abi.fp(b_map), abi.ip(b_cnt)))


ta, tb = [], []
ra, rb = np.full(2, -1, np.float32), np.full(2, -1, np.float32)
for i in range(WARM + REPS):
    ctx.sync(); t0 = time.perf_counter(); route_a(ra); t1 = time.perf_counter()
    ctx.sync(); t2 = time.perf_counter(); route_b(rb); t3 = time.perf_counter()
    if i >= WARM:
        ta.append(t1 - t0); tb.append(t3 - t2)
same = (np.array_equal(a_rgb, b_rgb) and np.array_equal(a_map.view(np.uint32), b_map.view(np.uint32)) and np.array_equal(a_cnt, b_cnt)
        and np.array_equal(ra.view(np.uint32), rb.view(np.uint32)))
ma, mb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
say("debugPlotIDepthMap + debugPlotIDepthMapFloat of one keyframe: host route (a) vs sdso_track_depth_image (b) on %s" % device_name())
say("%d calls each after %d warm-ups, the routes taking turns; %dx%d, %d points: pc_n[0] %d, allID.size() %d, %d circles, range %.6g .. %.6g"
    % (REPS, WARM, W, H, NPTS, pcn[0], b_cnt[0], b_cnt[1], rb[0], rb[1]))
say("images, map, range and counts identical: %s" % same)
say("  (a) host route             median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
say("      of which (medians): download of the %d-float map %.3f, C++ -O3 single thread %.3f ms"
    % ((W * H,) + tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0))))
say("  (b) sdso_track_depth_image median %.3f ms   (min %.3f), both images copied back (%d bytes)" % (mb, 1e3 * min(tb), W * H * 7 + 16))
say("  (a) / (b) = %.2f" % (ma / mb))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 2))
ctx.check(ctx.L.sdso_prof_reset(ctx.h))
for _ in range(10):
    route_b(rb)
ctx.sync()
tot = 0.0
for k in ("k_di_hist", "k_di_pick", "k_di_image"):
    ms, n = ctx.prof_read(k)
    tot += ms / 10
    say("  kernel (b): %-10s %.1f us x %d per call" % (k, 1e3 * ms / max(n, 1), n // 10))
say("  kernels (b) per call: %.1f us" % (1e3 * tot))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
ctx.close()
shutil.rmtree(tmp, ignore_errors=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not same:
    print("MISMATCH between the two routes")
    sys.exit(1)
