"""Times the hand-off between two contexts of one GPU (sdso_pyramid_export / _import, sdso_track_export_ref / _import_ref) against the
routes it replaces, in one process at 1232x368:
  per keyframe, the tracking template (about 4000 points) from the mapping ctx A to the tracking ctx B
    (a) sdso_track_export_ref on A + sdso_track_import_ref on B + the first sdso_track_calc_res_gs (level 0) on B
    (b) sdso_track_get_ref on A + sdso_track_set_ref on B over all levels + the same evaluation
  per frame, the stereo pair from the tracking ctx to the mapping ctx
    (c) sdso_pyramid_export + sdso_pyramid_import of both eyes, and the same followed by sdso_ctx_sync of the importer; in turns
        into slots that still view the last frame (the import then frees it, as its last holder) and into slots released beforehand
    (d) a second sdso_ingest_frame of the same raw pair on the importer + sdso_ctx_sync
    and the builder's next sdso_ingest_frame into slots it exported from (fresh level buffers) against slots nobody exported
  what freezing costs the builder: sdso_track_make_ref into a slot whose last template was exported and is still held by B
    (e) detached: fresh level buffers (the allocations of track_make_ref_dev)
    (f) in place: the same call into a slot nobody exported — the code path of the commit before the hand-off existed, unchanged by it
Everything above is measured twice in the same run, turn by turn: on a pair of contexts without a buffer pool, and on a second pair
attached to one sdso_pool (the pooled route: the frees of (c), the fresh buffers of the detached builds and of (e) become parks and
hand-outs behind stream waits).  The pool's counters are reported with it.
Median of --reps calls of each route after --warm warm-ups, the routes of a group taking turns; every timed window ends when the last
call returns.  What (a) and (b), (c) and (d) leave on the importer is compared bit for bit.
  python tools/time_handoff.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, is appended to FILE (profiles/handoff_timing.txt holds such reports).  There is no pass mark."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
from sdso_amd.params import track_params
import ingest_cases as Cs
import synth
import undistort_ref as R

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
W, H, NPTS = 1232, 368, 4000
REF_A, REF_A_OWN, REF_B, REF_B_HOST, NEW = 1, 2, 3, 4, 9
KEYS = ("u", "v", "idepth", "color")
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


def med(t):
    return "median %.3f ms   (min %.3f)" % (1e3 * float(np.median(t)), 1e3 * min(t))


prob = synth.tracker_problem(w=W, h=H, npts=NPTS, seed=2201)
L = prob["levels"]
u, v, idp = prob["points"]
ui, vi, idp = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32), np.ascontiguousarray(idp, np.float32)
wgt = np.random.RandomState(3).uniform(0.1, 30.0, NPTS).astype(np.float32)
prm = track_params(prob)
ev = abi.TrackEval()
abi.load().sdso_track_make_eval(C.byref(prm), 0, C.byref(abi.SE3.from_Rt(np.eye(3), np.zeros(3))), C.byref(abi.Aff(0, 0)), 1.0, C.byref(ev))
size = Cs.KITTI
raws = [Cs.raw_image(size["wOrg"], size["hOrg"], 8, 100 + i) for i in range(2)]
_, rx, ry, _ = R.make_remap(R.RADTAN, Cs.pars(R.RADTAN, size), size["wOrg"], size["hOrg"], W, H, R.CROP)
G, vinv = Cs.response(8), Cs.vignette_inv(size["wOrg"], size["hOrg"])


class Rig:
    """a mapping ctx A and a tracking ctx B of device 0, attached to `pool` (None: no pool), and the timings taken on them"""

    def __init__(self, pool):
        self.pool = pool
        self.A, self.B = abi.Context(0), abi.Context(0)
        if pool is not None:
            self.A.set_pool(pool); self.B.set_pool(pool)
        self.pcn = np.zeros(8, np.int32)
        for c in (self.A, self.B):
            c.upload_pyramid(NEW, prob["pyr_new"])
        self.A.upload_pyramid(NEW + 1, prob["pyr_ref"])
        self.ta, self.tb, self.te, self.tf, self.split_a = [], [], [], [], []
        self.tc, self.tcs, self.tce, self.td, self.tg, self.th = [], [], [], [], [], []
        self.same_tpl = self.same_pyr = True
        self.make_ref(REF_A); self.make_ref(REF_A_OWN)

    def make_ref(self, slot):
        A = self.A
        A.check(A.L.sdso_track_make_ref(A.h, slot, NEW + 1, NPTS, abi.ip(ui), abi.ip(vi), abi.fp(idp), abi.fp(wgt), abi.ip(self.pcn)))

    def get_ref(self, ctx, slot):
        out = []
        for l in range(L):
            nn = C.c_int(-1)
            ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), None, None, None, None))
            arrs = [np.zeros(nn.value, np.float32) for _ in KEYS]
            if nn.value:
                ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), *[abi.fp(a) for a in arrs]))
            out.append(arrs)
        return out

    def evaluate(self, slot):
        B = self.B
        Hm, b, res, nw = np.zeros(64), np.zeros(8), np.zeros(6), C.c_int(-1)
        B.check(B.L.sdso_track_calc_res_gs(B.h, slot, NEW, C.byref(ev), abi.dp(Hm), abi.dp(b), abi.dp(res), C.byref(nw), None))
        return Hm.tobytes() + b.tobytes() + res.tobytes(), nw.value

    def template_turn(self, i):
        """the template, per keyframe"""
        A, B = self.A, self.B
        A.sync(); B.sync()
        t0 = time.perf_counter()
        h = A.export_ref(REF_A)
        t1 = time.perf_counter()
        B.import_ref(REF_B, h)
        t2 = time.perf_counter()
        ra = self.evaluate(REF_B)
        t3 = time.perf_counter()
        h.release()
        A.sync(); B.sync()
        t4 = time.perf_counter()
        for l, arrs in enumerate(self.get_ref(A, REF_A)):
            B.check(B.L.sdso_track_set_ref(B.h, REF_B_HOST, l, len(arrs[0]), *[abi.fp(a) for a in arrs]))
        rb = self.evaluate(REF_B_HOST)
        t5 = time.perf_counter()
        self.same_tpl = self.same_tpl and ra == rb and ra[1] > 0
        # the builder's next keyframe: REF_A's levels are frozen and B still views them; REF_A_OWN was never exported
        A.sync()
        t6 = time.perf_counter(); self.make_ref(REF_A); t7 = time.perf_counter()
        A.sync()
        t8 = time.perf_counter(); self.make_ref(REF_A_OWN); t9 = time.perf_counter()
        if i >= WARM:
            self.ta.append(t3 - t0); self.tb.append(t5 - t4); self.te.append(t7 - t6); self.tf.append(t9 - t8); self.split_a.append((t1 - t0, t2 - t1, t3 - t2))

    def frames_begin(self):
        for c in (self.A, self.B):
            assert Cs.calib_create(c, 1, size, (rx, ry), 8, G, vinv, 2) == 0

    def frame_turn(self, i):
        """the stereo pair, per frame"""
        A, B = self.A, self.B
        # the builder's frame: slots 20 / 21 were exported last turn and B still views them (detached: fresh level buffers); 50 / 51 never were
        A.sync()
        t0 = time.perf_counter(); A.ingest_frame(1, (20, 21), raws, (0.01, 0.02)); A.sync(); t1 = time.perf_counter()
        A.ingest_frame(1, (50, 51), raws, (0.01, 0.02)); A.sync(); t2 = time.perf_counter()
        if i >= WARM:
            self.tg.append(t1 - t0); self.th.append(t2 - t1)
        empty = i % 2 == 1                                 # every second turn B has let the last frame go beforehand, outside the window
        if empty:
            for s in (30, 31):
                B.check(B.L.sdso_release_pyramid(B.h, s))
        A.sync(); B.sync()
        t0 = time.perf_counter()
        hs = [A.export_pyramid(s) for s in (20, 21)]
        for hh, s in zip(hs, (30, 31)):
            B.import_pyramid(s, hh)
        t1 = time.perf_counter()
        B.sync()
        t2 = time.perf_counter()
        for hh in hs:
            hh.release()
        t3 = time.perf_counter()
        B.ingest_frame(1, (40, 41), raws, (0.01, 0.02))
        B.sync()
        t4 = time.perf_counter()
        if i >= WARM:
            (self.tce if empty else self.tc).append(t1 - t0); self.tcs.append(t2 - t0); self.td.append(t4 - t3)
        if i == WARM:
            self.same_pyr = all(Cs.same_bits(Cs.download_pyramid(B, a, W, H), Cs.download_pyramid(B, b, W, H)) for a, b in ((30, 40), (31, 41)))

    def report(self, title):
        say(title)
        say("template per keyframe, %d points: pc_n %s; evaluation on the importer identical: %s" % (NPTS, [int(x) for x in self.pcn[:L]], self.same_tpl))
        say("  (a) export + import + first sdso_track_calc_res_gs   %s" % med(self.ta))
        say("      of which (medians): export %.3f, import %.3f, evaluation %.3f ms" % tuple(1e3 * np.median(np.array(self.split_a), axis=0)))
        say("  (b) sdso_track_get_ref + sdso_track_set_ref, all levels, + the evaluation   %s" % med(self.tb))
        say("  (b) / (a) = %.2f" % (float(np.median(self.tb)) / float(np.median(self.ta))))
        say("stereo pair per frame; pyramids on the importer identical: %s" % self.same_pyr)
        say("  (c) export + import of both eyes, the importer's slots still viewing the last frame as its last holder:")
        say("      the import %s that frame's %d level buffers    %s" % ("parks" if self.pool else "frees", 2 * L, med(self.tc)))
        say("      into slots the importer had released before      %s" % med(self.tce))
        say("      either + sdso_ctx_sync of the importer            %s" % med(self.tcs))
        say("  (d) second sdso_ingest_frame of the raw pair + sync   %s" % med(self.td))
        say("  what freezing costs the builder's next sdso_ingest_frame + sync of the pair:")
        say("      detached: %d %s level buffers                  %s" % (2 * L, "pooled" if self.pool else "fresh", med(self.tg)))
        say("      in place: slots nobody exported                   %s" % med(self.th))
        say("the builder's next sdso_track_make_ref (synchronous call) after an export that the importer still holds")
        say("  (e) detached: %s level buffers                     %s" % ("pooled" if self.pool else "fresh", med(self.te)))
        say("  (f) in place: a slot nobody exported                  %s" % med(self.tf))
        say("  (e) - (f) = %.3f ms per keyframe" % (1e3 * (float(np.median(self.te)) - float(np.median(self.tf)))))
        if self.pool:
            say("  the pool's counters at the end: %s" % self.pool.stats())


pool = abi.Pool(0, 1 << 30)
rigs = [Rig(None), Rig(pool)]
for i in range(WARM + REPS):
    for r in rigs:
        r.template_turn(i)
for r in rigs:
    r.frames_begin()
for i in range(WARM + 2 * REPS):                       # (c)'s two forms take turns: --reps calls of each
    for r in rigs:
        r.frame_turn(i)

say("hand-off between two contexts of %s, against the routes through the host, without and with a buffer pool; %dx%d" % (device_name(), W, H))
say("%d calls each after %d warm-ups, the routes of a group and the two pairs of contexts taking turns" % (REPS, WARM))
rigs[0].report("---- without a pool")
rigs[1].report("---- both contexts attached to one sdso_pool")
same_tpl, same_pyr = all(r.same_tpl for r in rigs), all(r.same_pyr for r in rigs)
for r in rigs:
    r.A.close(); r.B.close()
pool.release()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(("\n" if f.tell() else "") + "\n".join(lines) + "\n")
if not (same_tpl and same_pyr):
    print("MISMATCH between the routes")
    sys.exit(1)
