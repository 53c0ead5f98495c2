"""CPU statement of the device-resident immature-point set (sdso_imm_*): FullSystem::makeNewTraces (FullSystem.cpp:1600-1629),
traceNewCoarseKey / traceNewCoarseNonKey (:632-781) and STEP 5 of activatePointsMT (:948-957).

The per-point work is the oracle's (orc_immature_init_batch, orc_trace_on_batch, orc_trace_stereo_batch); the glue between the calls is
NumPy float32 in the operation order include/sdso_abi.h states: one rounding per operation, row products summed left to right (the
convention of oracle/orc_math.h and tests/distmap_ref.py).  A host's points are a dict of arrays, one entry per ImmaturePoint member."""
import ctypes as C

import numpy as np

from sdso_amd import abi

f32 = np.float32
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
FIELDS = ("u", "v", "my_type", "idepth_min", "idepth_max", "quality", "color", "weights", "gradH", "energyTH", "lastTraceStatus", "lastTraceUV",
          "lastTracePixelInterval")
# sdso_imm_trace's counts
C_FWD_GOOD, C_STEREO_OUTLIER, C_UPDATED, C_UNREADABLE = 6, 7, 8, 9


def _init(orc, img, u, v):
    """ImmaturePoint::ImmaturePoint (ImmaturePoint.cpp:33-88) at (u, v) of img [h, w, 3]."""
    h, w, _ = img.shape
    n = len(u)
    col, wgt, gH, eth = np.zeros((n, 8), f32), np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros(n, f32)
    if n:
        orc.orc_immature_init_batch(abi.fp(img), w, h, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth))
    return col, wgt, gH, eth


def add_frame(orc, img, selection_map):
    """makeNewTraces' loop (:1611-1626) on img [h, w, 3]: the host's points in raster order."""
    img = np.ascontiguousarray(img, f32)
    h, w, _ = img.shape
    m = np.asarray(selection_map, f32).reshape(h, w)
    inner = np.zeros((h, w), bool)
    inner[3:h - 4, 3:w - 4] = True
    ys, xs = np.nonzero(inner & (m != 0))            # np.nonzero walks rows first: raster order
    u, v = xs.astype(f32), ys.astype(f32)
    col, wgt, gH, eth = _init(orc, img, u, v)
    keep = np.isfinite(eth)                          # :1619
    n = int(keep.sum())
    return dict(u=u[keep], v=v[keep], my_type=m[ys, xs][keep].astype(f32), idepth_min=np.zeros(n, f32), idepth_max=np.full(n, np.nan, f32),
                quality=np.full(n, 10000, f32), color=col[keep], weights=wgt[keep], gradH=gH[keep], energyTH=eth[keep],
                lastTraceStatus=np.full(n, UNINITIALIZED, np.uint8), lastTraceUV=np.zeros((n, 2), f32), lastTracePixelInterval=np.zeros(n, f32))


def _points(n, u, v, col, wgt, gH, eth, idepth_min, imin_s, imax_s, quality=None, status=None, uv=None, interval=None):
    P, d = abi.make_trace_points(n, u, v, col, wgt, gH, eth, imin_s, imax_s)
    d["idepth_min"][:] = idepth_min
    if quality is not None:
        d["quality"][:] = quality; d["lastTraceStatus"][:] = status; d["lastTraceUV"][:] = uv; d["lastTracePixelInterval"][:] = interval
    return P, d


def _trace_stereo(orc, img, K4, baseline, mode_right, P, gn_mode):
    h, w, _ = img.shape
    st = np.zeros(P.n, np.uint8)
    if P.n:
        assert orc.orc_trace_stereo_batch_gn(abi.fp(img), w, h, abi.fp(K4), float(baseline), mode_right, C.byref(P), abi.bp(st), gn_mode) == 0
    return st


def _readable(uv, w, h):
    return (uv[:, 0] >= 2) & (uv[:, 1] >= 2) & (uv[:, 0] < w - 3) & (uv[:, 1] < h - 3)


def _project(G, u, v, idepth):
    """1 / (KRKi * (Vec3f(u, v, 1) / idepth) + Kt)[2]  (:675-679)"""
    KRKi, Kt = G["KRKi"], G["Kt"]
    with np.errstate(all="ignore"):
        x0, x1, x2 = u / idepth, v / idepth, f32(1) / idepth
        return f32(1) / (((KRKi[6] * x0 + KRKi[7] * x1) + KRKi[8] * x2) + Kt[2])


def _back_project(G, Ki, us, vs, s):
    """1 / (KRi * (Ki * Vec3f(us, vs, 1) / s - t))[2]  (:713-717)"""
    KRi, t = G["KRi"], G["t"]
    with np.errstate(all="ignore"):
        q = [(Ki[3 * k] * us + Ki[3 * k + 1] * vs) + Ki[3 * k + 2] * f32(1) for k in range(3)]
        p = [q[k] / s - t[k] for k in range(3)]
        return f32(1) / ((KRi[6] * p[0] + KRi[7] * p[1]) + KRi[8] * p[2])


def trace(orc, named, left, right, K4, Ki, baseline, gn_mode=0):
    """traceNewCoarseKey (right is None) / traceNewCoarseNonKey on the named hosts, in place.  named: list of (points, geom) with geom a
    dict of float32 arrays KRKi[9], Kt[3], aff[2], KRi[9], t[3].  Returns sdso_imm_trace's counts and, for the tests of the case itself,
    the histograms of the statuses traceOn and the forward traceStereo returned."""
    left = np.ascontiguousarray(left, f32)
    h, w, _ = left.shape
    K4 = np.ascontiguousarray(K4, f32)
    Ki = None if Ki is None else np.ascontiguousarray(Ki, f32).ravel()
    counts = np.zeros(abi.IMM_NCOUNTS, np.int32)
    on_hist, fwd_hist = np.zeros(6, np.int64), np.zeros(6, np.int64)
    for S, G in named:
        n = len(S["u"])
        if n == 0:
            continue
        # ---- traceOn (:669 / :769), on the host's own arrays
        P, d = _points(n, S["u"], S["v"], S["color"], S["weights"], S["gradH"], S["energyTH"], S["idepth_min"], S["idepth_min"], S["idepth_max"],
                       S["quality"], S["lastTraceStatus"], S["lastTraceUV"], S["lastTracePixelInterval"])
        g = abi.TraceGeom()
        g.KRKi[:] = [float(x) for x in G["KRKi"]]; g.Kt[:] = [float(x) for x in G["Kt"]]; g.aff[:] = [float(x) for x in G["aff"]]
        st = np.zeros(n, np.uint8)
        assert orc.orc_trace_on_batch(abi.fp(left), w, h, 1, C.byref(g), abi.ip(np.zeros(n, np.int32)), C.byref(P), abi.bp(st)) == 0
        assert np.array_equal(st, d["lastTraceStatus"])           # traceOn returns what it leaves in lastTraceStatus
        S["idepth_min"], S["idepth_max"], S["quality"] = d["idepth_min_stereo"], d["idepth_max_stereo"], d["quality"]
        S["lastTraceStatus"], S["lastTraceUV"], S["lastTracePixelInterval"] = d["lastTraceStatus"], d["lastTraceUV"], d["lastTracePixelInterval"]
        on_hist += np.bincount(st, minlength=6)[:6]
        if right is None:
            continue
        # ---- the stereo chain of the points traceOn returned GOOD for (:671-730)
        right = np.ascontiguousarray(right, f32)
        good = st == GOOD
        ok = good & _readable(S["lastTraceUV"], w, h)
        counts[C_UNREADABLE] += int((good & ~ok).sum())
        a = np.nonzero(ok)[0]
        pmin = _project(G, S["u"][a], S["v"][a], S["idepth_min"][a])
        pmax = _project(G, S["u"][a], S["v"][a], S["idepth_max"][a])
        fu, fv = S["lastTraceUV"][a, 0].copy(), S["lastTraceUV"][a, 1].copy()
        Pf, df = _points(len(a), fu, fv, *_init(orc, left, fu, fv), pmin, pmin, pmax)                   # :672-686
        sf = _trace_stereo(orc, right, K4, baseline, 1, Pf, gn_mode)                                     # :689
        fwd_hist += np.bincount(sf, minlength=6)[:6]
        fgood = sf == GOOD
        counts[C_FWD_GOOD] += int(fgood.sum())
        fok = fgood & _readable(df["lastTraceUV"], w, h)
        counts[C_UNREADABLE] += int((fgood & ~fok).sum())
        b = np.nonzero(fok)[0]
        bu, bv = df["lastTraceUV"][b, 0].copy(), df["lastTraceUV"][b, 1].copy()
        Pb, db = _points(len(b), bu, bv, *_init(orc, right, bu, bv), np.zeros(len(b), f32), pmin[b], pmax[b])   # :692-697
        _trace_stereo(orc, left, K4, baseline, 0, Pb, gn_mode)                                           # :700, status not examined
        us, vs = df["u_stereo"][b], df["v_stereo"][b]
        with np.errstate(all="ignore"):
            delta = np.abs(us - db["lastTraceUV"][:, 0])
            disparity = us - df["lastTraceUV"][b, 0]
            out = (delta > 1) & (disparity < 10)                                                         # :707
        S["lastTraceStatus"][a[b[out]]] = OUTLIER
        counts[C_STEREO_OUTLIER] += int(out.sum())
        upd = ~out
        S["idepth_min"][a[b[upd]]] = _back_project(G, Ki, us[upd], vs[upd], df["idepth_min_stereo"][b][upd])
        S["idepth_max"][a[b[upd]]] = _back_project(G, Ki, us[upd], vs[upd], df["idepth_max_stereo"][b][upd])
        counts[C_UPDATED] += int(upd.sum())
    for S, _ in named:
        counts[:6] += np.bincount(S["lastTraceStatus"], minlength=6)[:6].astype(np.int32)
    return counts, on_hist, fwd_hist


def remove_order(flags):
    """STEP 5 (:948-957) on a list of old indices; a flagged entry stands for the null pointer."""
    v = list(range(len(flags)))
    i = 0
    while i < len(v):
        if flags[v[i]]:
            v[i] = v[-1]
            v.pop()
            i -= 1
        i += 1
    return v


def remove(S, flags):
    src = np.array(remove_order(flags), np.int64)
    for k in FIELDS:
        S[k] = np.ascontiguousarray(S[k][src])


def same(a, b):
    """every member of two hosts' points, bit for bit (NaN equals NaN); returns the first member that differs, or None"""
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=(x.dtype != np.uint8)):
            return k
    return None
