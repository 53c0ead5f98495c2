"""Inputs whose discrete epipolar searches run past one wave of steps (64) and up to the 99-step cap of ImmaturePoint.cpp:267 / :650.

A search has numSteps = 1.9999f + dist steps, dist <= maxPixSearch = 0.027 (w + h), so the step count is a property of the image size:
wide, low images reach it at a fraction of the pixels of a KITTI frame.

    S1  2400 x 160   maxPixSearch  69.12   a fresh search has 71 steps          (second pass of the lane = step loops)
    S2  3840 x 160   maxPixSearch 108      a fresh search has 109 -> 99 steps   (second pass and the cap)

The right camera is 2.5 m away, so that the matches themselves lie past step 64.  Every render (about 2 s) is made once per process."""
import ctypes as C
import functools

import numpy as np

from sdso_amd import abi
import immature_cases as Cs
import synth

f32 = np.float32
S1, S2 = (2400, 160), (3840, 160)
BASELINE = 2.5
SEED = 4101                                   # points; the noise of the left / right image is SEED + 1 / SEED + 2
MOTION = (2.5, -0.03, 0.15, 0.002, -0.004, 0.003)
AFF = (0.02, 1.5)
TRACE_ON_SEED = 2141
FIELDS = ("idepth_min_stereo", "idepth_max_stereo", "idepth_stereo", "quality", "lastTraceStatus", "lastTraceUV", "lastTracePixelInterval")
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
RESIDENT_POINTS = 1003                        # not a multiple of 4 (points per traceOn workgroup) or 16 (per traceStereo workgroup)
PERIODIC_RESIDENT_POINTS = 503


def _K4(shape):
    cal = synth.kitti_calib(*shape)
    return np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"]], f32)


@functools.lru_cache(maxsize=None)
def _left(shape):
    """raw left image and its inverse depth"""
    return synth.Scene(1001).render(shape[0], shape[1], _K4(shape), (np.eye(3), np.zeros(3)), noise_seed=SEED + 1)


@functools.lru_cache(maxsize=None)
def _right(shape, baseline):
    return synth.Scene(1001).render(shape[0], shape[1], _K4(shape), (np.eye(3), np.array([-float(baseline), 0.0, 0.0])), noise_seed=SEED + 2)[0]


def _level0(img):
    return np.ascontiguousarray(synth.make_pyramid(img, 1)[0])


def oracle_init(orc, img, u, v):
    """ImmaturePoint::ImmaturePoint at (u, v) of img [h, w, 3]"""
    h, w, _ = img.shape
    n = len(u)
    col, wgt, gH, eth = np.zeros((n, 8), f32), np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros(n, f32)
    orc.orc_immature_init_batch(abi.fp(img), w, h, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth))
    return col, wgt, gH, eth


def oracle_trace(orc, case, img, P, mode_right, gn_mode=0):
    st = np.zeros(P.n, np.uint8)
    assert orc.orc_trace_stereo_batch_gn(abi.fp(img), case["w"], case["h"], abi.fp(case["K"]), case["baseline"], mode_right, C.byref(P), abi.bp(st), gn_mode) == 0
    return st


# ------------------------------------------------------------------ static stereo
@functools.lru_cache(maxsize=None)
def stereo_case(shape):
    """A stereo pair with a 2.5 m baseline and 3000 points on the left image; `idepth_min` / `idepth_max` are the finite intervals:
    55 ... maxPixSearch + 12 px long (clamped and unclamped searches), the true disparity 5 ... 95 % of the way along them."""
    w, h = shape
    K = _K4(shape)
    il, idl = _left(shape)
    L, R = _level0(il), _level0(_right(shape, BASELINE))
    u, v = synth.select_points(L, 3000, SEED, margin=6)
    idt = idl[v, u]
    u, v = u.astype(f32), v.astype(f32)
    n = len(u)
    fb = f32(K[0]) * f32(BASELINE)
    rs = np.random.RandomState(5)
    Lpx = rs.uniform(55, (w + h) * 0.027 + 12, n).astype(f32)
    frac = rs.uniform(0.05, 0.95, n).astype(f32)
    lo = np.maximum(fb * idt - frac * Lpx, f32(0.5))
    hi = lo + Lpx
    return dict(w=w, h=h, K=K, baseline=BASELINE, left=L, right=R, u=u, v=v, idepth_true=idt, idepth_min=(lo / fb).astype(f32), idepth_max=(hi / fb).astype(f32))


@functools.lru_cache(maxsize=None)
def periodic_case(period=64, tile_at=1800):
    """S2 with the usual 0.5372 m baseline, both images replaced by copies of their columns tile_at ... tile_at + period - 1.  The rows
    have that period and a fresh search steps by exactly -1 px, so step s + period samples the very values of step s: the best energy
    occurs more than once and the reference keeps the earliest (strictly smaller energies only, in step order).  With period 64 the equal
    steps s and s + 64 meet on one lane of the wave (the merge of a lane's two candidates); with period 32 the steps s and s + 32 lie on
    different lanes (the index rule of the reduction across lanes)."""
    w, h = S2
    bl = float(synth.kitti_calib(w, h)["baseline"])
    il, _ = _left(S2)
    ir = _right(S2, bl)
    L = _level0(np.tile(il[:, tile_at:tile_at + period], (1, w // period)))
    R = _level0(np.tile(ir[:, tile_at:tile_at + period], (1, w // period)))
    assert np.array_equal(R[:, period:2 * period, 0], R[:, 10 * period:11 * period, 0])
    u, v = synth.select_points(L, 500, SEED, margin=6, min_grad=4.0)
    return dict(w=w, h=h, K=_K4(S2), baseline=bl, left=L, right=R, u=u.astype(f32), v=v.astype(f32), period=period)


# every GOOD match of a periodic pair is the earliest of the equal steps.  Period 64: the bound the case was designed with.  Period 32: the
# earliest step is less than 32 px from the start and the refinement moves it by at most 3 steps of 0.5 px; a later one lies 32 px further.
MAX_PERIODIC_DISPARITY = {64: 63.5, 32: 33.5}


def max_pix_search(w, h):
    return f32(w + h) * f32(0.027)


def stereo_step_count(case, idepth_min=None, idepth_max=None):
    """numSteps of ImmaturePoint::traceStereo (mode_right) for points that reach the search, restated in float32 for a horizontal
    epipolar line (ImmaturePoint.cpp:118-267): uMin, uMax, dist, the clamp to maxPixSearch, int(1.9999f + dist), the cap 99.
    Returns (numSteps, uMin).  For the coverage conditions only; nothing is compared with it bit for bit."""
    u = case["u"]
    n = len(u)
    Kt0 = f32(case["K"][0]) * f32(-case["baseline"])
    mps = max_pix_search(case["w"], case["h"])
    imin = np.zeros(n, f32) if idepth_min is None else idepth_min.astype(f32)
    uMin = u + Kt0 * imin
    if idepth_max is None:
        dist = np.full(n, mps, f32)
    else:
        uMax = u + Kt0 * idepth_max.astype(f32)
        dist = np.sqrt((uMin - uMax) * (uMin - uMax))
        dist = np.minimum(dist, mps)
    steps = (f32(1.9999) + dist).astype(np.int32)
    return np.where(steps >= 100, 99, steps), uMin


# ------------------------------------------------------------------ traceOn
@functools.lru_cache(maxsize=None)
def _tracker(shape):
    return synth.tracker_problem(w=shape[0], h=shape[1], npts=3000, seed=TRACE_ON_SEED, motion=MOTION, aff=AFF)


def _geom(KRKi, Kt, aff):
    G = abi.TraceGeom()
    G.KRKi[:] = [float(x) for x in np.ravel(KRKi)]; G.Kt[:] = [float(x) for x in Kt]; G.aff[:] = [float(x) for x in aff]
    return G


def project0(KRKi, u, v):
    """where idepth = 0 projects to: the start of a fresh traceOn search"""
    KRKi = np.asarray(KRKi, f32).reshape(3, 3)
    p = (KRKi @ np.stack([u, v, np.ones(len(u), f32)])).T
    return p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]


@functools.lru_cache(maxsize=None)
def trace_on_case(shape):
    """A host keyframe and the newest frame 2.5 m to its side (plus a little of everything else, so the epipolar lines are neither
    horizontal nor parallel); geometry as _trace_on_case of test_stereo.py.  `geoms`: the true one and one with aff = (1, 0)."""
    prob = _tracker(shape)
    u, v, idp = prob["points"]
    R, t = prob["refToNew_true"]
    fx, fy, cx, cy = [f32(x) for x in prob["K"]]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    Ki = np.linalg.inv(K.astype(np.float64)).astype(f32)
    KRKi = (K @ R.astype(f32) @ Ki).astype(f32)
    Kt = (K @ t.astype(f32)).astype(f32)
    G = _geom(KRKi, Kt, (np.exp(f32(AFF[0])), AFF[1]))
    G2 = _geom(KRKi, Kt, (1.0, 0.0))
    return dict(w=shape[0], h=shape[1], host=np.ascontiguousarray(prob["pyr_ref"][0]), new=np.ascontiguousarray(prob["pyr_new"][0]),
                u=u.astype(f32), v=v.astype(f32), idepth_true=idp.astype(f32), KRKi=KRKi, Kt=Kt, G=G, geoms=(abi.TraceGeom * 2)(G, G2))


def trace_on_mixed_state(case):
    """Prior states as in test_gpu_trace_on_bit_exact: fresh, a finite interval, previously OOB / OUTLIER; every seventh point uses the
    second geometry.  The finite intervals are long: they end at 1.05 ... 2.5 times the true inverse depth and start at 0.3 ... 0.9
    times it or, every other one, at 0 ... 0.04 times it (at S1 a match lies at most 71.5 px from idepth = 0, so only an interval that
    starts next to 0 has its match past step 64).  Searches of more than 64 steps occur both below maxPixSearch and clamped to it."""
    n = len(case["u"])
    idp = case["idepth_true"]
    rs = np.random.RandomState(7)
    pg = (np.arange(n) % 7 == 0).astype(np.int32)
    imin = np.zeros(n, f32); imax = np.full(n, np.nan, f32)
    sel = np.arange(n) % 3 == 1
    lo = np.where(np.arange(n) % 6 == 1, rs.uniform(0.0, 0.04, n), rs.uniform(0.3, 0.9, n)).astype(f32)
    imin[sel] = (idp * lo)[sel]; imax[sel] = (idp * rs.uniform(1.05, 2.5, n).astype(f32))[sel]
    sel2 = np.arange(n) % 11 == 2
    imin[sel2] = idp[sel2] * f32(0.99); imax[sel2] = idp[sel2] * f32(1.01)
    prev = np.full(n, UNINITIALIZED, np.uint8); prev[np.arange(n) % 13 == 3] = OOB; prev[np.arange(n) % 13 == 4] = OUTLIER
    return dict(pg=pg, idepth_min=imin, idepth_max=imax, prev=prev, long_interval=sel & ~sel2)


def trace_on_interval_ends(case, idepth_min, idepth_max):
    """(uMin, vMin, dist before the clamp) of traceOn's interval with the first geometry, float32 (ImmaturePoint.cpp:480-520)"""
    KRKi, Kt = case["KRKi"], case["Kt"]
    pr = (KRKi @ np.stack([case["u"], case["v"], np.ones(len(case["u"]), f32)])).T.astype(f32)
    with np.errstate(all="ignore"):
        pmin = pr + Kt[None, :] * idepth_min[:, None]
        pmax = pr + Kt[None, :] * idepth_max[:, None]
        uMin, vMin = pmin[:, 0] / pmin[:, 2], pmin[:, 1] / pmin[:, 2]
        uMax, vMax = pmax[:, 0] / pmax[:, 2], pmax[:, 1] / pmax[:, 2]
        return uMin, vMin, np.sqrt((uMin - uMax) ** 2 + (vMin - vMax) ** 2)


@functools.lru_cache(maxsize=None)
def periodic_trace_on_case(period=64):
    """The periodic pair as a traceOn problem: the left image is the host, the right one the newest frame, hostToNew is the stereo
    translation alone (KRKi = I, Kt = K (-baseline, 0, 0), aff = (1, 0)).  A fresh search starts at the point itself and steps by exactly
    -1 px along the row, so step s + period has the energy of step s bit for bit, as in traceStereo.  `map`, `geom`, `K4`, `Ki`: the same
    problem for the resident set (sdso_imm_add_frame + the key form of sdso_imm_trace)."""
    case = periodic_case(period)
    w, h = case["w"], case["h"]
    cal, K4, K, Ki = Cs.calib(w, h)
    g = Cs.geom(K, Ki, (np.eye(3), np.zeros(3)), (np.eye(3), np.array([-case["baseline"], 0.0, 0.0])), (0.0, 0.0))
    assert np.array_equal(g["KRKi"], np.eye(3, dtype=f32).ravel()) and g["Kt"][1] == 0 and g["Kt"][2] == 0 and np.array_equal(g["aff"], [1, 0])
    G = _geom(g["KRKi"], g["Kt"], g["aff"])
    return dict(w=w, h=h, host=case["left"], new=case["right"], u=case["u"], v=case["v"], KRKi=g["KRKi"].reshape(3, 3), Kt=g["Kt"], G=G,
                geoms=(abi.TraceGeom * 1)(G), period=period, K4=K4, Ki=Ki.ravel().copy(), baseline=case["baseline"], geom=g,
                map=Cs.selection_map(case["left"], None, PERIODIC_RESIDENT_POINTS, 9, w=w, h=h))


# ------------------------------------------------------------------ the resident set
@functools.lru_cache(maxsize=None)
def resident_case():
    """S2: the host and the frame's left image are those of trace_on_case; the frame's right camera is 2.5 m from its left one."""
    w, h = S2
    prob = _tracker(S2)
    cal, K4, K, Ki = Cs.calib(w, h)
    T_host = (np.eye(3), np.zeros(3))
    T = prob["refToNew_true"]
    right, _ = synth.Scene(1001).render(w, h, K4, (T[0], T[1] + np.array([-BASELINE, 0.0, 0.0])), noise_seed=TRACE_ON_SEED + 13, aff=AFF)
    host = np.ascontiguousarray(prob["pyr_ref"][0])
    return dict(w=w, h=h, K4=K4, Ki=Ki.ravel().copy(), baseline=BASELINE, host=host, left=np.ascontiguousarray(prob["pyr_new"][0]), right=_level0(right),
                map=Cs.selection_map(host, None, RESIDENT_POINTS, 9, w=w, h=h), geom=Cs.geom(K, Ki, T_host, T, AFF))
