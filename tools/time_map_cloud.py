"""Times the published map of one keyframe (KeyFrameDisplay::setFromKF + refreshPC for the whole window, KeyFrameDisplay.cpp:85-165,
:174-295, as FullSystem.cpp:1467 publishes it) two ways in one process, at the workload's shape: 8 keyframes x 2000 points, half of them
active points of the resident BA window (8 x 1000), half in the marginalised / out lists earlier keyframes left:
  (a) what a caller does today: sdso_ba_get_post_state with the per-point arrays (idepth, idepth_hessian, maxRelBaseline are the
      values refreshPC filters on), the records of the active points rebuilt on the host, then tools/map_cloud_cpu.cpp — a C++ -O3
      single-thread statement of setFromKF + refreshPC — once per keyframe over the host's own copy of the lists
  (b) sdso_map_update (the active lists replaced from the resident window) + sdso_map_cloud over the 8 keyframes, arrays copied back
  (c) the same with SDSO_MAP_ONE_WAIT=1: sdso_map_cloud copies both arrays at their upper bound behind ONE wait instead of waiting for
      the counts and then for the used prefix — the variant (b) was chosen against
Median of --reps calls of each route after --warm warm-ups, the routes taking turns; every timed window ends when the call returns.
Vertices, colours and first[] of the routes are compared byte for byte.  The kernel times come from sdso_prof_read in a pass of
their own.
  python tools/time_map_cloud.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/map_cloud_timing.txt is such a report).  There is no pass mark: the result
is a latency to report."""
import ctypes as C
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
os.environ["SDSO_DEBUG_ENV"] = "1"            # the library's A/B switches are read only under this gate, which it reads once: route (c)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import map_ref as ref
import synth
import window_update_helpers as wu

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
WID, PER_KF = 13, 1000
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
tmp = tempfile.mkdtemp(prefix="map_cloud_cpu_")
lib = os.path.join(tmp, "libmap_cloud_cpu.so")
subprocess.check_call([os.environ.get("CXX") or shutil.which("g++") or "g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                       os.path.join(ROOT, "tools", "map_cloud_cpu.cpp"), "-o", lib])
cpu = C.CDLL(lib)
cpu.map_cloud_cpu.argtypes = [C.c_int, abi.c_float_p, abi.c_u8_p] + [C.c_float] * 7 + [C.c_int, abi.c_float_p, abi.c_u8_p]

win = synth.ba_window(w=1232, h=368, nf=8, pts_per_kf=PER_KF, seed=3001)
win = wu.with_history(win, 5)
nf, npts, nr = win["nf"], win["np"], win["nr"]
host = np.asarray(win["host"])
fids = [int(f) for f in win["frameID"]]

ctx = abi.Context(0)
wu.upload_pyramids(ctx, win)
keep = wu.upload(ctx, win, WID)
wu.optimize(ctx, WID)
post0 = wu.post_state(ctx, WID, win)
K4 = post0["calib_value_scaled"].astype(np.float32)
order = [np.asarray(l, np.int64) for l in ref.point_lists(host, nf)]   # fh->pointHessians of every frame, as index arrays: no route pays for a list
active = np.concatenate(order).astype(np.int32)
# what earlier keyframes left: per keyframe 500 marginalised and 500 out records, values drawn from the window's own
rs = np.random.RandomState(9)
old = {}
for h, fid in enumerate(fids):
    src = ref.records_from_post(win, post0, rs.choice(np.nonzero(host == h)[0], PER_KF))
    src[:, 0] += rs.uniform(-3, 3, PER_KF).astype(np.float32)
    old[fid] = {2: np.ascontiguousarray(src[:PER_KF // 2]), 3: np.ascontiguousarray(src[PER_KF // 2:])}
    ctx.map_put(fid, 2, old[fid][2]); ctx.map_put(fid, 3, old[fid][3])
ctx.map_update(WID, active, [], [])
frames = [dict(lists={1: ref.records_from_post(win, post0, order[h]), 2: old[fid][2], 3: old[fid][3]}) for h, fid in enumerate(fids)]
th = ref.quantile_thresholds(frames)
MODE = 1
total = sum(len(f["lists"][l]) for f in frames for l in (1, 2, 3))
cap = 8 * total

# (a): the per-point arrays of the post-state, and the host's own copy of the lists
post = dict(idepth=np.zeros(npts, np.float32), step=np.zeros(npts, np.float32), HdiF=np.zeros(npts, np.float32), bdSumF=np.zeros(npts, np.float32),
            idepth_hessian=np.zeros(npts, np.float32), maxRelBaseline=np.zeros(npts, np.float32), numGoodResiduals=np.zeros(npts, np.int32))
P = abi.BAPostState()
abi.bind(P, post)
a_rec = [np.concatenate([f["lists"][l] for l in (1, 2, 3)]) for f in frames]               # (the active part is rewritten per call)
a_status = [np.concatenate([np.full(len(f["lists"][l]), l, np.uint8) for l in (1, 2, 3)]) for f in frames]
a_xyz, a_rgb, a_first = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros(nf + 1, np.int32)
split = []


def route_a():
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_ba_get_post_state(ctx.h, WID, C.byref(P)))
    t1 = time.perf_counter()
    nv = 0
    for h in range(nf):
        idx = order[h]
        r = a_rec[h]
        r[:len(idx), 2] = post["idepth"][idx]; r[:len(idx), 3] = post["idepth_hessian"][idx]; r[:len(idx), 4] = post["maxRelBaseline"][idx]
        a_first[h] = nv
        nv += cpu.map_cloud_cpu(len(r), abi.fp(r), abi.bp(a_status[h]), K4[0], K4[1], K4[2], K4[3], th["scaledTH"], th["absTH"], th["minBS"], MODE,
                                abi.fp(a_xyz[nv:]), abi.bp(a_rgb[nv:]))
    a_first[nf] = nv
    split.append((t1 - t0, time.perf_counter() - t1))


U = abi.MapUpdate()
U.n_active = len(active); U.active = abi.ip(active); U.n_gone = 0; U.gone = None; U.gone_list = None
fid_a = np.ascontiguousarray(fids, np.int32)
Q = abi.MapCloud()
Q.n_frames = nf; Q.frameID = abi.ip(fid_a); Q.imm_host_id = None
Q.fx, Q.fy, Q.cx, Q.cy = [float(x) for x in K4]
Q.scaledTH, Q.absTH, Q.minBS, Q.mode = th["scaledTH"], th["absTH"], th["minBS"], MODE
Q.camToWorld = None; Q.cap = cap
b_xyz, b_rgb, b_first = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros(nf + 1, np.int32)
split_b = []


def route_b():
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_map_update(ctx.h, WID, C.byref(U)))
    t1 = time.perf_counter()
    ctx.check(ctx.L.sdso_map_cloud(ctx.h, C.byref(Q), abi.fp(b_xyz), abi.bp(b_rgb), abi.ip(b_first), None))
    split_b.append((t1 - t0, time.perf_counter() - t1))


c_xyz, c_rgb, c_first = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros(nf + 1, np.int32)
split_c = []


def route_c():
    os.environ["SDSO_MAP_ONE_WAIT"] = "1"
    t0 = time.perf_counter()
    ctx.check(ctx.L.sdso_map_update(ctx.h, WID, C.byref(U)))
    t1 = time.perf_counter()
    ctx.check(ctx.L.sdso_map_cloud(ctx.h, C.byref(Q), abi.fp(c_xyz), abi.bp(c_rgb), abi.ip(c_first), None))
    split_c.append((t1 - t0, time.perf_counter() - t1))
    del os.environ["SDSO_MAP_ONE_WAIT"]


ta, tb, tc = [], [], []
for i in range(WARM + REPS):
    ctx.sync(); t0 = time.perf_counter(); route_a(); t1 = time.perf_counter()
    ctx.sync(); t2 = time.perf_counter(); route_b(); t3 = time.perf_counter()
    ctx.sync(); route_c()
    if i >= WARM:
        ta.append(t1 - t0); tb.append(t3 - t2); tc.append(sum(split_c[-1]))
n = int(b_first[nf])
same = (np.array_equal(a_first, b_first) and np.array_equal(a_xyz[:n].view(np.uint32), b_xyz[:n].view(np.uint32)) and np.array_equal(a_rgb[:n], b_rgb[:n])
        and np.array_equal(c_first, b_first) and np.array_equal(c_xyz[:n].view(np.uint32), b_xyz[:n].view(np.uint32)) and np.array_equal(c_rgb[:n], b_rgb[:n]))
ma, mb = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
say("setFromKF + refreshPC of the whole window at one keyframe: host route (a) vs sdso_map_update + sdso_map_cloud (b) on %s" % device_name())
say("%d calls each after %d warm-ups, the routes taking turns; 8 keyframes x %d records (%d active in the window, %d in the marginalised / out lists), mode %d: %d of %d points kept, %d vertices"
    % (REPS, WARM, total // nf, npts, total - npts, MODE, n // 8, total, n))
say("vertices, colours and first[] identical: %s" % same)
say("  (a) host route                          median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
say("      of which (medians): sdso_ba_get_post_state (7 per-point arrays) %.3f, records + C++ -O3 single thread %.3f ms"
    % tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0)))
say("  (b) sdso_map_update + sdso_map_cloud    median %.3f ms   (min %.3f), %d bytes copied back" % (mb, 1e3 * min(tb), 15 * n + 128))
say("      of which (medians): sdso_map_update (enqueue only) %.3f, sdso_map_cloud %.3f ms" % tuple(1e3 * np.median(np.array(split_b[WARM:WARM + REPS]), axis=0)))
say("  (a) / (b) = %.2f" % (ma / mb))
mc = 1e3 * float(np.median(tc))
say("  (c) the same, SDSO_MAP_ONE_WAIT=1       median %.3f ms   (min %.3f), %d bytes copied back (the upper bound), one wait" % (mc, 1e3 * min(tc), 15 * cap + 128))
say("      of which (medians): sdso_map_update %.3f, sdso_map_cloud %.3f ms" % tuple(1e3 * np.median(np.array(split_c[WARM:WARM + REPS]), axis=0)))
say("  (c) / (b) = %.2f" % (mc / mb))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 2))
ctx.check(ctx.L.sdso_prof_reset(ctx.h))
for _ in range(10):
    route_b()
ctx.sync()
tot = 0.0
for k in ("k_map_gather", "k_map_mark", "k_map_emit"):
    ms, cnt = ctx.prof_read(k)
    tot += ms / 10
    say("  kernel (b): %-12s %.1f us x %d per call" % (k, 1e3 * ms / max(cnt, 1), cnt // 10))
say("  kernels (b) per call: %.1f us" % (1e3 * tot))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
ctx.check(ctx.L.sdso_ba_release_window(ctx.h, WID))
ctx.check(ctx.L.sdso_map_clear(ctx.h))
ctx.close()
shutil.rmtree(tmp, ignore_errors=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not same:
    print("MISMATCH between the two routes")
    sys.exit(1)
