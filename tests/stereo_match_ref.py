"""CPU statement of sdso_imm_stereo_match: the loop of FullSystem::stereoMatch (FullSystem.cpp:581-613) on one group of the resident
immature points, a dict of arrays as tests/immature_ref.py keeps it.

The per-point work is the oracle's (immature_ref._points, _init, _trace_stereo, _readable); the glue is NumPy float32 with one rounding
per operation.  The group is not changed."""
import numpy as np

import immature_ref as R

f32 = np.float32
NOT_RUN = 255
NCOUNTS = 8
C_WALKED, C_FWD_GOOD, C_BACK_RUN, C_BACK_GOOD, C_ACCEPTED, C_FAR, C_DEPTH, C_UNREADABLE = range(NCOUNTS)
RESULT = ("accepted", "idepth", "status_fwd", "status_back")


def stereo_match(orc, S, left, right, K4, baseline, max_depth=70.0, gn_mode=0):
    """-> dict(accepted [n] u8, idepth [n, 3], status_fwd [n], status_back [n], counts [8], map [h, w, 3]) and, for a test that walks the
    points itself, the raw outputs of the two traces: fwd [n, 3] (idepth_stereo, idepth_min_stereo, idepth_max_stereo), back_u [n]."""
    left, right = np.ascontiguousarray(left, f32), np.ascontiguousarray(right, f32)
    h, w, _ = left.shape
    K4 = np.ascontiguousarray(K4, f32)
    return match_with(S, w, h, lambda u, v: R._init(orc, right, u, v),
                      lambda P, in_right: R._trace_stereo(orc, right if in_right else left, K4, baseline, 1 if in_right else 0, P, gn_mode), max_depth)


def match_with(S, w, h, init_right, trace, max_depth=70.0):
    """The loop on a group with the per-point work handed in: init_right(u, v) -> the members ImmaturePoint::ImmaturePoint gives a point of
    the right image; trace(P, in_right) -> the statuses of traceStereo on the points P, searched in the right image (mode_right 1) or in
    the left one (mode_right 0)."""
    n = len(S["u"])
    zeros, nan = np.zeros(n, f32), np.full(n, np.nan, f32)
    # ---- :582-587: the point itself, its interval reset, searched in the right image
    Pf, df = R._points(n, S["u"], S["v"], S["color"], S["weights"], S["gradH"], S["energyTH"], zeros, zeros, nan, S["quality"], S["lastTraceStatus"],
                       S["lastTraceUV"], S["lastTracePixelInterval"])
    sf = trace(Pf, True)
    fgood = sf == R.GOOD
    fok = fgood & R._readable(df["lastTraceUV"], w, h)
    # ---- :589-596: a fresh point of the right image at lastTraceUV, searched in the left one
    b = np.nonzero(fok)[0]
    bu, bv = df["lastTraceUV"][b, 0].copy(), df["lastTraceUV"][b, 1].copy()
    Pb, db = R._points(len(b), bu, bv, *init_right(bu, bv), np.zeros(len(b), f32), np.zeros(len(b), f32), np.full(len(b), np.nan, f32))
    sb = np.full(n, NOT_RUN, np.uint8)
    sb[b] = trace(Pb, False)
    back_u = np.full(n, np.nan, f32)
    back_u[b] = db["lastTraceUV"][:, 0]
    # ---- :598-601
    fwd = np.stack([df["idepth_stereo"], df["idepth_min_stereo"], df["idepth_max_stereo"]], axis=1).astype(f32)
    with np.errstate(all="ignore"):
        delta = np.abs(np.asarray(S["u"], f32) - back_u)
        depth = f32(1) / fwd[:, 0]
        near = delta < 1
        in_range = (depth > 0) & (depth < f32(max_depth))
    bgood = sb == R.GOOD
    acc = bgood & near & in_range
    idepth = np.where(acc[:, None], fwd, f32(0)).astype(f32)
    counts = np.zeros(NCOUNTS, np.int32)
    counts[C_WALKED], counts[C_FWD_GOOD], counts[C_BACK_RUN], counts[C_BACK_GOOD] = n, fgood.sum(), fok.sum(), bgood.sum()
    counts[C_ACCEPTED], counts[C_FAR], counts[C_DEPTH] = acc.sum(), (bgood & ~near).sum(), (bgood & near & ~in_range).sum()
    counts[C_UNREADABLE] = (fgood & ~fok).sum()
    # ---- :606-608 as a dense image; a point whose pixel is not in the image writes nothing
    m = np.zeros((h, w, 3), f32)
    u, v = np.asarray(S["u"], f32), np.asarray(S["v"], f32)
    with np.errstate(all="ignore"):
        inside = acc & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    for i in np.nonzero(inside)[0]:
        m[int(v[i]), int(u[i])] = idepth[i]
    return dict(accepted=acc.astype(np.uint8), idepth=idepth, status_fwd=sf, status_back=sb, counts=counts, map=m, fwd=fwd, back_u=back_u)


def same(a, b, keys=RESULT + ("counts", "map")):
    """two results bit for bit (NaN equals NaN); returns the first member that differs, or None"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=(x.dtype != np.uint8 and x.dtype != np.int32)):
            return k
    return None
