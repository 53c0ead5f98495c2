"""Times the per-frame immature-point path (traceNewCoarseNonKey) at the workload's own shape: 1232x368, 7 host keyframes x 3000
candidates, 4 successive stereo frames, two ways in one process with alternating repetitions:
  (a) the composed path: sdso_trace_on_batch on host arrays, NumPy glue (select GOOD, project the interval), sdso_stereo_match_batch,
      the accept rule and the interval update on the host
  (b) sdso_imm_trace on the device-resident set (counts == NULL)
Each timed window is one frame and ends in sdso_ctx_sync.  The host state / the set is rebuilt untimed before every repetition, so both
paths do identical work; their final states are compared bit for bit.  On a library without sdso_imm_* (the parent commit) only (a)
runs: that is the baseline.  Prints the report; profiles/immature_resident_ab.txt holds the output of both commits.
  python tools/time_immature.py [--reps N] [--prof] [--only-a]
--prof: kernel times from HIP events, in loops of their own: k_trace_on / k_trace_stereo of path (a), then the kernels of (b).
--only-a: path (a) alone on this library too, as on the parent commit (no rebuild of the set between its repetitions)."""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import synth

f32 = np.float32
W, H, NHOST, NCAND, NFRAME = 1232, 368, 7, 3000, 4
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
HAVE_IMM = hasattr(abi, "ImmGeom") and "--only-a" not in sys.argv
FIELDS = ("u", "v", "idepth_min", "idepth_max", "quality", "color", "weights", "gradH", "energyTH", "lastTraceStatus", "lastTraceUV", "lastTracePixelInterval")

cal = synth.kitti_calib(W, H)
K4 = np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"]], f32)
K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], f32)
Ki = np.linalg.inv(K.astype(np.float64)).astype(f32)
Ki9 = np.ascontiguousarray(Ki.ravel())
BL = float(cal["baseline"])
sc = synth.Scene(1001)
pose = lambda k: synth.se3_exp(np.array([0.02 * k, -0.005 * k, 0.8 * k, 0.001 * k, -0.002 * k, 0.001 * k], np.float64))


def geom(Th, Tf, aff):
    R, t = synth.se3_mul(Tf, synth.se3_inv(Th))
    R, t = R.astype(f32), t.astype(f32)
    return dict(KRKi=(K @ R @ Ki).astype(f32).ravel(), Kt=(K @ t).astype(f32), aff=np.array([np.exp(aff[0]), aff[1]], f32), KRi=(K @ R.T).astype(f32).ravel(), t=t)


ctx = abi.Context(0)
L = ctx.L
hosts, frames = [], []
for k in range(NHOST):
    img, idp = sc.render(W, H, K4, pose(k), noise_seed=100 + k)
    dI = np.ascontiguousarray(synth.make_pyramid(img, 1)[0])
    u, v = synth.select_points(dI, NCAND, 200 + k, idepth=idp, min_idepth=0.0075)
    m = np.zeros((H, W), f32); m[v, u] = 1
    ctx.upload_pyramid(10 + k, [dI])
    ys, xs = np.nonzero(m)                                    # raster order, as makeNewTraces walks the map
    u, v = xs.astype(f32), ys.astype(f32)
    col, wgt, gH, eth = np.zeros((NCAND, 8), f32), np.zeros((NCAND, 8), f32), np.zeros((NCAND, 4), f32), np.zeros(NCAND, f32)
    ctx.check(L.sdso_immature_init_batch(ctx.h, 10 + k, NCAND, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
    assert np.isfinite(eth).all()
    hosts.append(dict(T=pose(k), map=m, u=u, v=v, color=col, weights=wgt, gradH=gH, energyTH=eth))
for k in range(NFRAME):
    T = pose(NHOST - 1 + 0.3 * (k + 1))
    aff = (0.01 * (k + 1), 0.5 * (k + 1))
    Tr = (T[0], T[1] + np.array([-BL, 0.0, 0.0]))
    l, _ = sc.render(W, H, K4, T, noise_seed=300 + 2 * k, aff=aff)
    r, _ = sc.render(W, H, K4, Tr, noise_seed=301 + 2 * k, aff=aff)
    ctx.upload_pyramid(30 + 2 * k, [synth.make_pyramid(l, 1)[0]]); ctx.upload_pyramid(31 + 2 * k, [synth.make_pyramid(r, 1)[0]])
    frames.append(dict(geom=[geom(h_["T"], T, aff) for h_ in hosts]))
N = NHOST * NCAND
PG = np.repeat(np.arange(NHOST, dtype=np.int32), NCAND)
cat = lambda k: np.ascontiguousarray(np.concatenate([h_[k] for h_ in hosts]))


def fresh_host_state():
    return dict(u=cat("u"), v=cat("v"), color=cat("color"), weights=cat("weights"), gradH=cat("gradH"), energyTH=cat("energyTH"),
                idepth_min=np.zeros(N, f32), idepth_max=np.full(N, np.nan, f32), quality=np.full(N, 10000, f32), lastTraceStatus=np.full(N, 5, np.uint8),
                lastTraceUV=np.zeros((N, 2), f32), lastTracePixelInterval=np.zeros(N, f32))


def frame_a(S, k):
    """the composed path of today on host arrays S; returns the wall time of the frame"""
    t0 = time.perf_counter()
    G = (abi.TraceGeom * NHOST)()
    for j, g in enumerate(frames[k]["geom"]):
        G[j].KRKi[:] = g["KRKi"].tolist(); G[j].Kt[:] = g["Kt"].tolist(); G[j].aff[:] = g["aff"].tolist()
    P = abi.TracePoints()
    P.n = N
    P.u_stereo, P.v_stereo, P.idepth_min_stereo, P.idepth_max_stereo = abi.fp(S["u"]), abi.fp(S["v"]), abi.fp(S["idepth_min"]), abi.fp(S["idepth_max"])
    P.color, P.weights, P.gradH, P.energyTH, P.quality = abi.fp(S["color"]), abi.fp(S["weights"]), abi.fp(S["gradH"]), abi.fp(S["energyTH"]), abi.fp(S["quality"])
    P.lastTraceStatus, P.lastTraceUV, P.lastTracePixelInterval = abi.bp(S["lastTraceStatus"]), abi.fp(S["lastTraceUV"]), abi.fp(S["lastTracePixelInterval"])
    st = np.zeros(N, np.uint8)
    ctx.check(L.sdso_trace_on_batch(ctx.h, 30 + 2 * k, NHOST, G, abi.ip(PG), C.byref(P), abi.bp(st)))
    uv = S["lastTraceUV"]
    a = np.nonzero((st == 0) & (uv[:, 0] >= 2) & (uv[:, 1] >= 2) & (uv[:, 0] < W - 3) & (uv[:, 1] < H - 3))[0]
    n = len(a)
    if n:
        KRKi = np.stack([g["KRKi"] for g in frames[k]["geom"]])[PG[a]]; Kt2 = np.stack([g["Kt"] for g in frames[k]["geom"]])[PG[a], 2]
        with np.errstate(all="ignore"):
            proj = []
            for key in ("idepth_min", "idepth_max"):
                d = S[key][a]
                proj.append(f32(1) / (((KRKi[:, 6] * (S["u"][a] / d) + KRKi[:, 7] * (S["v"][a] / d)) + KRKi[:, 8] * (f32(1) / d)) + Kt2))
        pmin, pmax = np.ascontiguousarray(proj[0]), np.ascontiguousarray(proj[1])
        fu, fv = np.ascontiguousarray(uv[a, 0]), np.ascontiguousarray(uv[a, 1])
        M = abi.StereoMatch()
        o = dict(status_fwd=np.zeros(n, np.uint8), idepth_min_out=np.zeros(n, f32), idepth_max_out=np.zeros(n, f32), fwd_uv=np.zeros((n, 2), f32), back_uv=np.zeros((n, 2), f32))
        M.n = n; M.u = abi.fp(fu); M.v = abi.fp(fv)
        M.idepth_min_stereo = abi.fp(pmin); M.idepth_max_stereo = abi.fp(pmax); M.back_idepth_min_stereo = abi.fp(pmin); M.back_idepth_max_stereo = abi.fp(pmax)
        abi.bind(M, o)
        ctx.check(L.sdso_stereo_match_batch(ctx.h, 30 + 2 * k, 31 + 2 * k, abi.fp(K4), BL, 1, C.byref(M)))
        b = np.nonzero(o["status_fwd"] == 0)[0]
        with np.errstate(all="ignore"):
            out = (np.abs(fu[b] - o["back_uv"][b, 0]) > 1) & (fu[b] - o["fwd_uv"][b, 0] < 10)
            S["lastTraceStatus"][a[b[out]]] = 2
            up = b[~out]
            KRi = np.stack([g["KRi"] for g in frames[k]["geom"]])[PG[a[up]]]; t = np.stack([g["t"] for g in frames[k]["geom"]])[PG[a[up]]]
            q = [(Ki9[3 * r] * fu[up] + Ki9[3 * r + 1] * fv[up]) + Ki9[3 * r + 2] * f32(1) for r in range(3)]
            for key, src in (("idepth_min", "idepth_min_out"), ("idepth_max", "idepth_max_out")):
                p = [q[r] / o[src][up] - t[:, r] for r in range(3)]
                S[key][a[up]] = f32(1) / ((KRi[:, 6] * p[0] + KRi[:, 7] * p[1]) + KRi[:, 8] * p[2])
    ctx.sync()
    return time.perf_counter() - t0


def rebuild_set():
    for j in range(NHOST):
        ctx.check(L.sdso_imm_release_host(ctx.h, j))
        n = C.c_int(0)
        ctx.check(L.sdso_imm_add_frame(ctx.h, j, 10 + j, abi.fp(hosts[j]["map"]), C.byref(n)))
        assert n.value == NCAND
    ctx.sync()


def frame_b(k):
    t0 = time.perf_counter()
    G = (abi.ImmGeom * NHOST)()
    for j, g in enumerate(frames[k]["geom"]):
        G[j].host_id = j
        for key in ("KRKi", "Kt", "aff", "KRi", "t"):
            getattr(G[j], key)[:] = g[key].tolist()
    ctx.check(L.sdso_imm_trace(ctx.h, 30 + 2 * k, 31 + 2 * k, NHOST, G, abi.fp(K4), abi.fp(Ki9), BL, None))
    ctx.sync()
    return time.perf_counter() - t0


ta, tb = [], []
Sa = None
for rep in range(REPS + 2):                       # two warm-up repetitions
    Sa = fresh_host_state()
    ra = [frame_a(Sa, k) for k in range(NFRAME)]
    if HAVE_IMM:
        rebuild_set()
        rb = [frame_b(k) for k in range(NFRAME)]
    if rep >= 2:
        ta.append(ra)
        if HAVE_IMM:
            tb.append(rb)
print("immature points per frame: %d x %d, %d hosts x %d points, %d stereo frames, %d repetitions after 2 warm-ups; wall time per frame in microseconds" %
      (W, H, NHOST, NCAND, NFRAME, REPS))
print("statuses after the last frame (GOOD OOB OUTLIER SKIPPED BADCONDITION UNINITIALIZED):", np.bincount(Sa["lastTraceStatus"], minlength=6)[:6])


def report(name, t):
    t = np.array(t) * 1e6
    for k in range(NFRAME):
        print("  %-44s frame %d: median %8.1f   min %8.1f   max %8.1f" % (name, k + 1, np.median(t[:, k]), t[:, k].min(), t[:, k].max()))
    print("  %-44s all %d : median %8.1f   min %8.1f   max %8.1f" % (name, NFRAME, np.median(t.sum(1)), t.sum(1).min(), t.sum(1).max()))


report("(a) trace_on_batch + glue + stereo_match_batch", ta)
if HAVE_IMM:
    report("(b) sdso_imm_trace on the resident set", tb)
    same = True
    for j in range(NHOST):
        d = ctx.imm_get(j)
        for key in FIELDS:
            x, y = d[key], Sa[key][j * NCAND:(j + 1) * NCAND]
            same &= bool(np.array_equal(x, y, equal_nan=x.dtype != np.uint8))
    print("final state of (b) equals (a) bit for bit:", same)
else:
    print("(path (a) only: --only-a, or a library without sdso_imm_* — the baseline)")
if "--prof" in sys.argv:
    # the kernels of path (a) alone, nothing of (b) in between: k_trace_on is the kernel whose body the resident path shares
    ctx.check(L.sdso_prof_reset(ctx.h)); ctx.check(L.sdso_prof_enable(ctx.h, 1))
    for rep in range(5):
        S = fresh_host_state()
        for k in range(NFRAME):
            frame_a(S, k)
    ctx.check(L.sdso_prof_enable(ctx.h, 0))
    print("kernel times of (a) from HIP events, microseconds per launch (launches):")
    for name in ("k_trace_on", "k_trace_stereo"):
        ms, n = ctx.prof_read(name)
        print("  %-22s %8.1f  (%d)" % (name, ms * 1e3 / max(n, 1), n))
    if HAVE_IMM:
        ctx.check(L.sdso_prof_reset(ctx.h)); ctx.check(L.sdso_prof_enable(ctx.h, 2))
        for rep in range(3):
            rebuild_set()
            for k in range(NFRAME):
                frame_b(k)
        ctx.check(L.sdso_prof_enable(ctx.h, 0))
        print("kernel times of (b) from HIP events, microseconds per launch (launches):")
        for name in ("k_imm_trace_on", "k_imm_stereo_prepare", "k_immature_init", "k_trace_stereo", "k_imm_back_points", "k_imm_accept", "k_imm_map_count", "k_imm_scan",
                     "k_imm_map_write", "k_imm_keep_count", "k_imm_keep_write"):
            ms, n = ctx.prof_read(name)
            if n:
                print("  %-22s %8.1f  (%d)" % (name, ms * 1e3 / n, n))
ctx.close()
