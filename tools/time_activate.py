"""Times activatePointsMT STEP 2-5 at the workload's own shape: 1232x368, 7 host keyframes x 3000 immature points after three traced
stereo frames, the last frame's left image as the newest keyframe (nf = 8), two ways in one process with alternating repetitions:
  (a) the composed path: sdso_imm_get of every host, flattening, sdso_activate_select, sdso_activate_points_batch, one sdso_imm_remove
      per host
  (b) sdso_imm_activate + sdso_imm_activate_fetch on the device-resident set
Each timed window ends in sdso_ctx_sync.  Before every repetition the set is rebuilt (release, add_frame, the traces) and the distance
map is made, untimed, so both paths do identical work; their records and final states are compared bit for bit.  Path (a) uses only
entry points that exist without sdso_imm_activate: on such a library (the parent commit) only (a) runs — the baseline.
  python tools/time_activate.py [--reps N] [--prof] [--only-a] [--mad currentMinActDist]
--prof: kernel times from HIP events, in loops of their own.  (k_activate_points of path (a) is launched without an event bracket:
its time comes from `rocprofv3 --kernel-trace --stats -- python tools/time_activate.py --only-a`.)"""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import distmap_cases as DC
import synth

f32 = np.float32
W, H, NHOST, NCAND, NFRAME = 1232, 368, 7, 3000, 3
NF = NHOST + 1
arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS = arg("--reps", 9, int)
MAD = arg("--mad", 3.0, float)
MIN_OBS = 1
HAVE_ACT = hasattr(abi, "ImmActivate") and "--only-a" not in sys.argv
FIELDS = ("u", "v", "my_type", "idepth_min", "idepth_max", "quality", "color", "weights", "gradH", "energyTH", "lastTraceStatus", "lastTraceUV", "lastTracePixelInterval")
REC = ("frame", "index", "status", "idepth", "res_state", "u", "v", "my_type", "idepth_min", "idepth_max", "energyTH", "color", "weights", "lastTraceStatus")

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
    m = np.zeros((H, W), f32); m[v, u] = np.array([1, 2, 4], f32)[np.arange(NCAND) % 3]
    ctx.upload_pyramid(10 + k, [dI])
    hosts.append(dict(T=pose(k), map=m))
for k in range(NFRAME):
    T = pose(NHOST - 1 + 0.3 * (k + 1))
    aff = (0.01 * (k + 1), 0.5 * (k + 1))
    Tr = (T[0], T[1] + np.array([-BL, 0.0, 0.0]))
    l, _ = sc.render(W, H, K4, T, noise_seed=300 + 2 * k, aff=aff)
    r, _ = sc.render(W, H, K4, Tr, noise_seed=301 + 2 * k, aff=aff)
    ctx.upload_pyramid(30 + 2 * k, [synth.make_pyramid(l, 1)[0]]); ctx.upload_pyramid(31 + 2 * k, [synth.make_pyramid(r, 1)[0]])
    frames.append(dict(T=T, aff=aff, geom=[geom(h_["T"], T, aff) for h_ in hosts]))
# the window: the hosts and the last frame's left image as the newest keyframe
Ts = [h_["T"] for h_ in hosts] + [frames[-1]["T"]]
affs = [(0.0, 0.0)] * NHOST + [frames[-1]["aff"]]
SLOTS = [10 + k for k in range(NHOST)] + [30 + 2 * (NFRAME - 1)]
IDS = list(range(NHOST)) + [NHOST]
pair_R, pair_t, pair_aff = np.zeros((NF * NF, 9), f32), np.zeros((NF * NF, 3), f32), np.zeros((NF * NF, 2), f32)
for h in range(NF):
    for t in range(NF):
        Rm, tv = synth.se3_mul(Ts[t], synth.se3_inv(Ts[h]))
        pair_R[h * NF + t] = Rm.astype(f32).ravel(); pair_t[h * NF + t] = tv.astype(f32)
        a = np.exp(affs[t][0] - affs[h][0])
        pair_aff[h * NF + t] = (a, affs[t][1] - a * affs[h][1])
KRKi, Kt = DC.window_geoms(np.array([synth.se3_pack(x) for x in Ts]), tuple(float(x) for x in K4))
FLAGGED = np.zeros(NF, np.uint8); FLAGGED[0] = 1
SLOTS_A = np.ascontiguousarray(SLOTS, np.int32)


def rebuild_set():
    """release, makeNewTraces, two non-key frames and the key frame: the state activatePointsMT meets (untimed)"""
    for j in range(NHOST):
        ctx.check(L.sdso_imm_release_host(ctx.h, j))
        n = C.c_int(0)
        ctx.check(L.sdso_imm_add_frame(ctx.h, j, 10 + j, abi.fp(hosts[j]["map"]), C.byref(n)))
        assert n.value == NCAND
    for k in range(NFRAME):
        G = (abi.ImmGeom * NHOST)()
        for j, g in enumerate(frames[k]["geom"]):
            G[j].host_id = j
            for key in ("KRKi", "Kt", "aff", "KRi", "t"):
                getattr(G[j], key)[:] = g[key].tolist()
        ctx.check(L.sdso_imm_trace(ctx.h, 30 + 2 * k, 31 + 2 * k if k + 1 < NFRAME else -1, NHOST, G, abi.fp(K4), abi.fp(Ki9), BL, None))
    ctx.sync()


rebuild_set()
S0 = [ctx.imm_get(j) for j in range(NHOST)]
# the active points behind the map: every 7th immature point with a finite interval, at its middle
pg, su, sv, sid = [], [], [], []
for j, S in enumerate(S0):
    i = np.arange(NCAND)[::7]
    i = i[np.isfinite(S["idepth_max"][i]) & np.isfinite(S["idepth_min"][i])]
    pg.append(np.full(len(i), j, np.int32)); su.append(S["u"][i]); sv.append(S["v"][i]); sid.append(f32(0.5) * (S["idepth_max"][i] + S["idepth_min"][i]))
SEEDS = [np.ascontiguousarray(np.concatenate(x)) for x in (pg, su, sv, sid)]


def make_map():
    return DC.dm_make(ctx, W, H, KRKi, Kt, *SEEDS)


def call_a():
    """the composed path; returns (wall time, decision, records)"""
    t0 = time.perf_counter()
    got = [ctx.imm_get(j) for j in range(NHOST)]
    cat = lambda k: np.ascontiguousarray(np.concatenate([S[k] for S in got]))
    frame = np.repeat(np.arange(NHOST, dtype=np.int32), [len(S["u"]) for S in got])
    index = np.concatenate([np.arange(len(S["u"]), dtype=np.int32) for S in got])
    cand = dict(pg=frame, u=cat("u"), v=cat("v"), idepth_min=cat("idepth_min"), idepth_max=cat("idepth_max"), quality=cat("quality"),
                interval=cat("lastTracePixelInterval"), status=cat("lastTraceStatus"), my_type=cat("my_type"))
    sel = DC.dm_select(ctx, dict(w=W, h=H, KRKi=KRKi, Kt=Kt, flagged=FLAGGED[:NHOST], cand=cand, min_act_dist=MAD, min_trace_quality=3.0))
    dec = sel["decision"]
    opt = np.nonzero(dec == 2)[0]
    ns = len(opt)
    rec = dict(frame=frame[opt], index=index[opt])
    for k in ("u", "v", "my_type", "idepth_min", "idepth_max", "energyTH", "color", "weights", "lastTraceStatus"):
        rec[k] = np.ascontiguousarray(cand[k][opt] if k in cand else cat(k)[opt])
    status, idepth, res_state = np.zeros(ns, np.int8), np.zeros(ns, f32), np.zeros((ns, NF), np.uint8)
    if ns:
        A = abi.Activate()
        A.nf, A.w, A.h, A.n, A.minObs = NF, W, H, ns, MIN_OBS
        A.K[:] = K4.tolist()
        A.pair_R, A.pair_t, A.pair_aff = abi.fp(pair_R), abi.fp(pair_t), abi.fp(pair_aff)
        A.u, A.v, A.idepth_min, A.idepth_max, A.color, A.weights, A.energyTH = [abi.fp(rec[k]) for k in ("u", "v", "idepth_min", "idepth_max", "color", "weights", "energyTH")]
        hs = np.ascontiguousarray(rec["frame"], np.int32)
        A.host = abi.ip(hs)
        A.frame_slot = abi.ip(SLOTS_A)
        ctx.check(L.sdso_activate_points_batch(ctx.h, C.byref(A), abi.ptr(status), abi.fp(idepth), abi.bp(res_state)))
    rec.update(status=status, idepth=idepth, res_state=res_state)
    flags = dec == 1
    flags[opt] = (status != 0) | (rec["lastTraceStatus"] == 1)
    o = 0
    for j, S in enumerate(got):
        n = len(S["u"])
        fl = np.ascontiguousarray(flags[o:o + n], np.uint8)
        ctx.check(L.sdso_imm_remove(ctx.h, j, n, abi.bp(fl)))
        o += n
    ctx.sync()
    return time.perf_counter() - t0, dec, rec


def call_b():
    t0 = time.perf_counter()
    counts, rec = ctx.imm_activate(IDS, SLOTS, FLAGGED, KRKi, Kt, pair_R, pair_t, pair_aff, W, H, K4, MIN_OBS, MAD)
    ctx.sync()
    return time.perf_counter() - t0, counts, rec


ta, tb = [], []
for rep in range(REPS + 2):                       # two warm-up repetitions
    rebuild_set(); make_map()
    da, dec_a, rec_a = call_a()
    state_a = [ctx.imm_get(j) for j in range(NHOST)]
    map_a = DC.dm_get(ctx, W, H)
    if HAVE_ACT:
        rebuild_set(); make_map()
        db, counts_b, rec_b = call_b()
    if rep >= 2:
        ta.append(da)
        if HAVE_ACT:
            tb.append(db)
print("activatePointsMT STEP 2-5: %d x %d, %d hosts x %d points after %d traced frames, nf = %d, currentMinActDist %.2f, minObs %d; %d repetitions after 2 warm-ups; "
      "wall time per call in microseconds" % (W, H, NHOST, NCAND, NFRAME, NF, MAD, MIN_OBS, REPS))
print("candidates %d: KEEP %d DELETE %d SELECT %d; statuses -1 / 0 / 1: %d / %d / %d; points left per host: %s" %
      (len(dec_a), (dec_a == 0).sum(), (dec_a == 1).sum(), (dec_a == 2).sum(), (rec_a["status"] == -1).sum(), (rec_a["status"] == 0).sum(), (rec_a["status"] == 1).sum(),
       [len(S["u"]) for S in state_a]))


def report(name, t):
    t = np.array(t) * 1e6
    print("  %-62s median %9.1f   min %9.1f   max %9.1f" % (name, np.median(t), t.min(), t.max()))
    return float(np.median(t))


med_a = report("(a) imm_get x7 + activate_select + activate_points_batch + imm_remove x7", ta)
if HAVE_ACT:
    med_b = report("(b) sdso_imm_activate + sdso_imm_activate_fetch", tb)
    same = bool(np.array_equal(dec_a, rec_b["decision"])) and bool(np.array_equal(map_a, DC.dm_get(ctx, W, H)))
    for k in REC:
        same &= bool(np.array_equal(rec_a[k], rec_b[k], equal_nan=rec_a[k].dtype == np.float32))
    for j in range(NHOST):
        d = ctx.imm_get(j)
        for key in FIELDS:
            same &= bool(np.array_equal(d[key], state_a[j][key], equal_nan=d[key].dtype != np.uint8))
    print("decisions, records, map and final state of (b) equal (a) bit for bit:", same)
else:
    print("(path (a) only: --only-a, or a library without sdso_imm_activate — the baseline)")
if "--prof" in sys.argv:
    def kernels(names):
        out = {}
        for name in names:
            ms, n = ctx.prof_read(name)
            if n:
                out[name] = (ms * 1e3 / n, n)
                print("  %-22s %9.1f  (%d)" % (name, ms * 1e3 / n, n))
        return out
    ctx.check(L.sdso_prof_reset(ctx.h)); ctx.check(L.sdso_prof_enable(ctx.h, 0))
    for rep in range(5):
        rebuild_set(); make_map()
        ctx.check(L.sdso_prof_reset(ctx.h) if rep == 0 else 0); ctx.check(L.sdso_prof_enable(ctx.h, 2))
        call_a()
        ctx.check(L.sdso_prof_enable(ctx.h, 0))
    print("kernel times of (a) from HIP events, microseconds per launch (launches):")
    ka = kernels(("k_select_classify", "k_distmap_select", "k_imm_gather"))
    print("  (a) median minus k_distmap_select: %9.1f" % (med_a - ka["k_distmap_select"][0]))
    if HAVE_ACT:
        for rep in range(5):
            rebuild_set(); make_map()
            ctx.check(L.sdso_prof_reset(ctx.h) if rep == 0 else 0); ctx.check(L.sdso_prof_enable(ctx.h, 2))
            call_b()
            ctx.check(L.sdso_prof_enable(ctx.h, 0))
        print("kernel times of (b) from HIP events, microseconds per launch (launches):")
        kb = kernels(("k_imm_act_classify", "k_distmap_select", "k_imm_act_list", "k_imm_activate", "k_imm_act_prefix", "k_imm_act_order", "k_imm_act_gather"))
        print("  (b) median minus k_distmap_select: %9.1f" % (med_b - kb["k_distmap_select"][0]))
ctx.close()
