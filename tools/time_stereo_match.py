"""Times the loop of FullSystem::stereoMatch (FullSystem.cpp:581-613) after makeNewTraces two ways in one process, at 1232x368 with the
selector's own points (sdso_pixel_select + sdso_imm_add_frame):
  (a) the route over the host: sdso_imm_get (every member of every point), sdso_stereo_match_batch on u, v (six uploads at most, seven
      downloads), then the accept rule and the scatter into the idepth image in numpy
  (b) sdso_imm_stereo_match, once with the per-point results alone (b1) and once with the dense map copied back as well (b2)
Median of --reps calls of each route after --warm warm-ups, the routes taking turns; every timed window ends when the call returns.
The results of the routes are compared byte for byte.  The kernel times come from sdso_prof_read in a pass of its own.
  python tools/time_stereo_match.py [--reps N] [--warm N] [--density D] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/stereo_match_resident_ab.txt is such a report).  There is no pass mark: the
result is a latency to report."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import immature_cases as Cs
import synth

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, DENSITY, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--density", 1500.0, float), arg("--out", None, str)
W, H = 1232, 368
SLOT_L, SLOT_R, HOST = 1, 2, 1
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


cal, K4, K, Ki = Cs.calib(W, H)
baseline = float(cal["baseline"])
T = synth.se3_exp(np.array(Cs.MOTIONS[0], np.float64))
(left, _), (right, _) = Cs.images(synth.Scene(1001), K4, T, Cs.NOISE[0], aff=Cs.AFFS[0], baseline=baseline, w=W, h=H)
pyr = synth.make_pyramid(np.ascontiguousarray(left[..., 0]))

ctx = abi.Context(0)
L = ctx.L
ctx.upload_pyramid(SLOT_L, pyr); ctx.upload_pyramid(SLOT_R, [right])
pot = C.c_int(3); num = C.c_int(0)
ctx.check(L.sdso_pixel_select(ctx.h, SLOT_L, DENSITY, 1, 1.0, C.byref(pot), None, C.byref(num)))
nn = C.c_int(0)
ctx.check(L.sdso_imm_add_frame(ctx.h, HOST, SLOT_L, None, C.byref(nn)))
n = nn.value

# (a)
mo = dict(status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), idepth_stereo=np.zeros(n, f32), idepth_min_out=np.zeros(n, f32),
          idepth_max_out=np.zeros(n, f32), fwd_uv=np.zeros((n, 2), f32), back_uv=np.zeros((n, 2), f32))
split = []


def route_a():
    t0 = time.perf_counter()
    S = ctx.imm_get(HOST)
    t1 = time.perf_counter()
    Mb = abi.StereoMatch()
    Mb.n = n; Mb.u = abi.fp(S["u"]); Mb.v = abi.fp(S["v"])
    abi.bind(Mb, mo)
    ctx.check(L.sdso_stereo_match_batch(ctx.h, SLOT_L, SLOT_R, abi.fp(K4), baseline, 1, C.byref(Mb)))
    t2 = time.perf_counter()
    with np.errstate(all="ignore"):
        depth = f32(1) / mo["idepth_stereo"]
        acc = (mo["status_fwd"] == 0) & (mo["status_back"] == 0) & (np.abs(S["u"] - mo["back_uv"][:, 0]) < 1) & (depth > 0) & (depth < f32(70))
    idepth = np.where(acc[:, None], np.stack([mo["idepth_stereo"], mo["idepth_min_out"], mo["idepth_max_out"]], axis=1), f32(0)).astype(f32)
    m = np.zeros((H, W, 3), f32)
    m[S["v"][acc].astype(np.int64), S["u"][acc].astype(np.int64)] = idepth[acc]
    split.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
    return acc.astype(np.uint8), idepth, m


O1, d1, c1 = ctx.imm_match_arrays(n, statuses=False)
O2, d2, c2 = ctx.imm_match_arrays(n, W, H, statuses=False)


def route_b1():
    ctx.check(L.sdso_imm_stereo_match(ctx.h, HOST, SLOT_L, SLOT_R, abi.fp(K4), baseline, 70.0, 0, C.byref(O1), abi.ip(c1)))
    return d1["accepted"], d1["idepth"]


def route_b2():
    ctx.check(L.sdso_imm_stereo_match(ctx.h, HOST, SLOT_L, SLOT_R, abi.fp(K4), baseline, 70.0, 1, C.byref(O2), abi.ip(c2)))
    return d2["accepted"], d2["idepth"], d2["map"]


ta, tb1, tb2 = [], [], []
for i in range(WARM + REPS):
    ctx.sync(); t0 = time.perf_counter(); ra = route_a(); t1 = time.perf_counter()
    ctx.sync(); t2 = time.perf_counter(); rb1 = route_b1(); t3 = time.perf_counter()
    ctx.sync(); t4 = time.perf_counter(); rb2 = route_b2(); t5 = time.perf_counter()
    if i >= WARM:
        ta.append(t1 - t0); tb1.append(t3 - t2); tb2.append(t5 - t4)
same = all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb2)) and all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb1))
ma, mb1, mb2 = (1e3 * float(np.median(t)) for t in (ta, tb1, tb2))
say("stereoMatch's loop after makeNewTraces: host route (a) vs sdso_imm_stereo_match (b) on %s" % device_name())
say("%d calls each after %d warm-ups, the routes taking turns; %dx%d, density %g: %d points" % (REPS, WARM, W, H, DENSITY, n))
say("counts (walked, fwd GOOD, back run, back GOOD, accepted, |du| >= 1, depth, unreadable): %s, results identical: %s" % (c2.tolist(), same))
say("  (a)  host route                       median %.3f ms   (min %.3f)" % (ma, 1e3 * min(ta)))
say("       of which (medians): sdso_imm_get %.3f, sdso_stereo_match_batch %.3f, rule and scatter in numpy %.3f ms"
    % tuple(1e3 * np.median(np.array(split[WARM:WARM + REPS]), axis=0)))
say("  (b1) sdso_imm_stereo_match, per point  median %.3f ms   (min %.3f)   (a) / (b1) = %.2f" % (mb1, 1e3 * min(tb1), ma / mb1))
say("  (b2) ... and the dense map copied back median %.3f ms   (min %.3f)   (a) / (b2) = %.2f" % (mb2, 1e3 * min(tb2), ma / mb2))
ctx.check(L.sdso_prof_enable(ctx.h, 2))
ctx.check(L.sdso_prof_reset(ctx.h))
for _ in range(10):
    route_b2()
ctx.sync()
for k in ("k_imm_match_prepare", "k_trace_stereo", "k_imm_match_back", "k_immature_init", "k_imm_match_accept"):
    ms, cnt = ctx.prof_read(k)
    say("  kernel (b2): %-20s %.1f us x %d per call" % (k, 1e3 * ms / max(cnt, 1), cnt // 10))
ctx.check(L.sdso_prof_enable(ctx.h, 0))
ctx.check(L.sdso_imm_release_host(ctx.h, HOST))
ctx.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not same:
    print("MISMATCH between the routes")
    sys.exit(1)
