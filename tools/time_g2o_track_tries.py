"""Times sdso_g2o_track_new_coarse — the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511) around the fork-live
trackNewestCoarse, resident on the device — against the only route a caller had before it, in one process, on the benchmark's tracking
problem (1232x368, 2000 points):
  (a) a list of five tries that stops at try 0 (lastCoarseRMSE large: the path of nearly every frame) against the host-driven single call
      sdso_g2o_track_newest_coarse on the same slots from the same start;
  (b) lists of 5, 27 and 53 tries that never stop (lastCoarseRMSE = 0) against a host loop of sdso_g2o_track_newest_coarse single calls
      under the carried bounds (the loop of tests/track_tries_ref.py, driven from Python like the call it is compared with).
      The lists are the reference's: the start, then the rotations Quaterniond(1, +-d, +-d, +-d) for d = 0.02 and 0.04 (:313-341);
  (c) the kernel's own time (k_g2o_track_lm between its events) for a batch of one and of 52, and the CPU oracle's time for one try.
Median of --reps calls of each route after --warm warm-ups, the two routes taking turns; every timed window ends when the call returns.
  python tools/time_g2o_track_tries.py [--reps N] [--warm N] [--out FILE]
The report goes to stdout and, with --out, to FILE (profiles/g2o_track_tries_timing.txt is such a report).  There is no pass mark."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import helpers
import synth
import track_tries_cases as cases
import track_tries_ref as ref
import g2o_track_tries_cases as g2o

arg = lambda name, default, conv: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
REPS, WARM, OUT = arg("--reps", 50, int), arg("--warm", 5, int), arg("--out", None, str)
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


def quat_pose(w, x, y, z):
    """SE3(Sophus::Quaterniond(w, x, y, z), 0): the quaternion is normalised by the constructor"""
    q = np.array([w, x, y, z], np.float64); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return tuple(R.reshape(9)) + (0.0, 0.0, 0.0)


def reference_tries():
    """the 53 tries of FullSystem.cpp:311-341"""
    out = [quat_pose(1, 0, 0, 0)]
    for d in (0.02, 0.04):
        for s in ((d, 0, 0), (0, d, 0), (0, 0, d), (-d, 0, 0), (0, -d, 0), (0, 0, -d), (d, d, 0), (0, d, d), (d, 0, d), (-d, d, 0), (0, -d, d), (-d, 0, d),
                  (d, -d, 0), (0, d, -d), (d, 0, -d), (-d, -d, 0), (0, -d, -d), (-d, 0, -d), (-d, -d, -d), (-d, -d, d), (-d, d, -d), (-d, d, d), (d, -d, -d),
                  (d, -d, d), (d, d, -d), (d, d, d)):
            out.append(quat_pose(1, *s))
    return out


prob = synth.tracker_problem(w=1232, h=368, npts=2000, seed=2002)                 # configs[1] of bench.py
ctx = abi.Context(0)
ctx.upload_pyramid(cases.NEW_SLOT, prob["pyr_new"]); ctx.set_ref(cases.REF_SLOT, prob["pc"])
prm = helpers.track_params(prob)
AFF0 = (0.0, 0.0)
TRIES = reference_tries()
assert len(TRIES) == 53


def single(T0, aff0, bounds):
    p = abi.TrackParams.from_buffer_copy(bytes(prm))
    for i in range(5):
        p.minResForAbort[i] = bounds[i]
    T = cases.se3_of(T0); aff = abi.Aff(*aff0); o = abi.TrackResult()
    ctx.check(ctx.L.sdso_g2o_track_newest_coarse(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(p), C.byref(T), C.byref(aff), C.byref(o)))
    return T, aff, o


class DeviceTracker:
    """sdso_g2o_track_newest_coarse behind the tracker interface of track_tries_ref: the host loop a caller had to write"""
    lastResiduals = [float("nan")] * 5
    lastFlowIndicators = [1000.0] * 3

    def trackNewestCoarse(self, _rec, lastToNew, aff_g2l, minResForAbort):
        T, aff, o = single(lastToNew, aff_g2l, minResForAbort)
        self.lastResiduals = list(o.lastResiduals); self.lastFlowIndicators = list(o.lastFlowIndicators)
        return bool(o.good), cases.se3_tuple(T), (aff.a, aff.b), -1


def host_loop(tries, rmse):
    return ref.track_new_coarse([None] * len(tries), tries, AFF0, rmse, 1.5, tracker=DeviceTracker())


def new_coarse(tries, rmse):
    rc, out, rm, R = g2o.new_coarse(ctx, prm, tries, AFF0, rmse, with_recs=False)
    ctx.check(rc)
    return out


def turns(fa, fb):
    ta, tb = [], []
    for i in range(WARM + REPS):
        ctx.sync(); t0 = time.perf_counter(); ra = fa(); t1 = time.perf_counter()
        ctx.sync(); t2 = time.perf_counter(); rb = fb(); t3 = time.perf_counter()
        if i >= WARM:
            ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t3 - t2))
    return np.array(ta), np.array(tb), ra, rb


say("sdso_g2o_track_new_coarse on %s: 1232x368, 2000 points, %d calls per route after %d warm-ups, the routes taking turns" % (device_name(), REPS, WARM))
# (a): everything a call does not write is built outside the timed windows, for both routes alike
T0_bytes, T5 = bytes(cases.se3_of(TRIES[0])), (abi.SE3 * 5)(*[cases.se3_of(t) for t in TRIES[:5]])
aff0_c = abi.Aff(*AFF0)


def single_a():
    T = abi.SE3.from_buffer_copy(T0_bytes); aff = abi.Aff(*AFF0); o = abi.TrackResult()
    ctx.check(ctx.L.sdso_g2o_track_newest_coarse(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(prm), C.byref(T), C.byref(aff), C.byref(o)))
    return T, aff, o


def new_coarse_a():
    out = abi.TrackTriesResult(); rm = (C.c_double * 5)(1e9, 1e9, 1e9, 1e9, 1e9)
    ctx.check(ctx.L.sdso_g2o_track_new_coarse(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(prm), 5, T5, C.byref(aff0_c), rm, 1.5, C.byref(out), None))
    return out


ta, tb, ra, rb = turns(single_a, new_coarse_a)
assert rb.tryIterations == 1 and rb.winner == 0
h = REPS // 2
say("(a) five tries, the loop stops at try 0 (evaluations %d, point evaluations %d)" % (ra[2].evaluations, ra[2].point_evals))
say("    sdso_g2o_track_newest_coarse  median %.4f ms   min %.4f   (minima of the two halves %.4f / %.4f)" % (np.median(ta), ta.min(), ta[:h].min(), ta[h:].min()))
say("    sdso_g2o_track_new_coarse     median %.4f ms   min %.4f   (minima of the two halves %.4f / %.4f)" % (np.median(tb), tb.min(), tb[:h].min(), tb[h:].min()))
say("    ratio of the medians %.2f; |pose difference| %.2e, level-0 residual %.6f / %.6f"
    % (np.median(ta) / np.median(tb), np.abs(np.array(cases.se3_tuple(ra[0])) - np.array(cases.se3_tuple(rb.pose))).max(), ra[2].lastResiduals[0], rb.achievedRes[0]))
ok = True
for n in (5, 27, 53):
    ta, tb, ra, rb = turns(lambda: host_loop(TRIES[:n], [0.0] * 5), lambda: new_coarse(TRIES[:n], [0.0] * 5))
    same = (ra["winner"], ra["tryIterations"], ra["haveOneGood"]) == (rb.winner, rb.tryIterations, rb.haveOneGood)
    tie = ra["winner"] >= 0 and rb.winner >= 0 and abs(ra["achievedRes"][0] - rb.achievedRes[0]) <= 1e-5 * ra["achievedRes"][0]
    ok = ok and (same or tie)
    say("(b) %2d tries, never stops: host loop of single calls median %.3f ms (min %.3f) | sdso_g2o_track_new_coarse median %.3f ms (min %.3f) | ratio %.2f"
        % (n, np.median(ta), ta.min(), np.median(tb), tb.min(), np.median(ta) / np.median(tb)))
    say("       winner %d / %d, tries run %d / %d, achievedRes[0] %.6f / %.6f%s" % (ra["winner"], rb.winner, ra["tryIterations"], rb.tryIterations, ra["achievedRes"][0],
                                                                                     rb.achievedRes[0], "" if same else "  (another winner within the tie of 1e-5)" if tie else "  MISMATCH"))
# (c) the kernel between its own events; the CPU oracle on the same try
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 1))
for n in (1, 52):
    ctx.check(ctx.L.sdso_prof_reset(ctx.h))
    for _ in range(WARM + REPS):
        rc, T, A, O = g2o.batch(ctx, [prm] * n, TRIES[:n], [AFF0] * n)
        ctx.check(rc)
    ms, launches = ctx.prof_read("k_g2o_track_lm")
    say("(c) k_g2o_track_lm, a batch of %2d: %.4f ms per launch over %d launches" % (n, ms / max(launches, 1), launches))
ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
try:
    import pyoracle
    orc = pyoracle.load()
    t_or = []
    for _ in range(5):
        t0 = time.perf_counter(); g2o.oracle_single(orc, prob, prm, TRIES[0], AFF0); t_or.append(1e3 * (time.perf_counter() - t0))
    say("(c) the CPU oracle (orc_g2o_track_newest_coarse, one host thread), one try: median %.1f ms" % np.median(t_or))
except Exception as e:                    # the oracle is test infrastructure: the report stands without it
    say("(c) the CPU oracle was not available: %s" % e)
ctx.close()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
if not ok:
    print("MISMATCH between the two routes")
    sys.exit(1)
