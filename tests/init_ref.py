"""CPU statement of the stereo initialiser (sdso_init_*): CoarseInitializer::setFirstStereo, level 0 (CoarseInitializer.cpp:842-972) and
STEP 3 of FullSystem::initializeFromInitializer (FullSystem.cpp:1533-1573).

The per-point work is the oracle's (orc_pixel_select, immature_ref._init, _points, _trace_stereo); the glue — which pixels become Pnts, what
a Pnt holds, which Pnts become points — is NumPy.  set_first_with / from_initializer take the per-point results as arguments, so the two
rules can be walked without a trace."""
import ctypes as C

import numpy as np

from sdso_amd import abi
import immature_ref as R

f32 = np.float32
NCOUNTS = 8
C_MAP, C_PNTS, C_HIST = 0, 1, 2
S_WALKED, S_SKIPPED, S_DROPPED, S_MADE = range(4)
PNT = ("u", "v", "idepth", "iR", "my_type", "status")
KEPT = ("energyTH", "idepth_min", "idepth_max", "idepth_stereo", "color", "weights")
POINT = ("pnt", "u", "v", "my_type", "idepth", "idepth_min", "idepth_max", "energyTH", "color", "weights")


def select(orc, pyr, density):
    """a fresh PixelSelector with currentPotential = 3, makeMaps(firstFrame, statusMap, density, 1, false, 2) (:848-871) -> (npts, map)"""
    keep = [np.ascontiguousarray(pyr[l], f32) for l in range(3)]
    ptrs = (abi.c_float_p * 3)(*[abi.fp(a) for a in keep])
    h, w, _ = keep[0].shape
    m = np.zeros((h, w), f32)
    p = C.c_int(3)
    n = orc.orc_pixel_select(ptrs, w, h, density, 1, 2.0, C.byref(p), abi.fp(m))
    return n, m


def candidates(selection_map):
    """the loop bounds of :892-896: y in [3, h-4), x in [3, w-4), raster order -> (x, y, map value)"""
    m = np.asarray(selection_map, f32)
    h, w = m.shape
    inner = np.zeros((h, w), bool)
    inner[3:h - 4, 3:w - 4] = True
    ys, xs = np.nonzero(inner & (m != 0))            # rows first: raster order
    return xs, ys, m[ys, xs].astype(f32)


def trace_first(orc, left, right, K4, baseline, gn_mode=0):
    """-> trace(u, v): ImmaturePoint(x, y, firstFrame, type) with the interval 0 / NaN, traceStereo(firstRightFrame, K, 1) (:897-903)"""
    left, K4 = np.ascontiguousarray(left, f32), np.ascontiguousarray(K4, f32)
    # A point with a NaN among its colours finds no best step, and the reference (and the oracle with it) then refines around (0, 0): it reads
    # pixels (-2, -2) ff., up to 2 rows and 2 pixels in front of the searched image.  The values cannot change the result (energyTH is NaN:
    # IPS_OUTLIER, or IPS_OOB from the line tests), but the memory must be there: the image is handed over with three rows of zeros before it.
    h, w, _ = np.shape(right)
    padded = np.zeros((h + 3, w, 3), f32)
    padded[3:] = right
    right = padded[3:]

    def trace(u, v):
        n = len(u)
        col, wgt, gH, eth = R._init(orc, left, u, v)
        P, d = R._points(n, u, v, col, wgt, gH, eth, np.zeros(n, f32), np.zeros(n, f32), np.full(n, np.nan, f32))
        st = R._trace_stereo(orc, right, K4, baseline, 1, P, gn_mode)
        return dict(status=st, energyTH=eth, idepth_min=d["idepth_min_stereo"], idepth_max=d["idepth_max_stereo"], idepth_stereo=d["idepth_stereo"], color=col,
                    weights=wgt)
    return trace


def set_first_with(selection_map, trace):
    """setFirstStereo's level-0 loop with the per-point work handed in: trace(u, v) -> dict of `status` and KEPT for float pixel arrays.
    -> dict(n, counts [8], pnts = dict of PNT, kept = dict of KEPT)"""
    xs, ys, ty = candidates(selection_map)
    u, v = xs.astype(f32), ys.astype(f32)
    t = trace(u, v)
    st = np.asarray(t["status"], np.uint8)
    good = st == R.GOOD
    idepth = np.where(good, np.asarray(t["idepth_stereo"], f32), f32(0.01)).astype(f32)      # :910-911 / :945-947
    counts = np.zeros(NCOUNTS, np.int32)
    counts[C_MAP], counts[C_PNTS] = (np.asarray(selection_map) != 0).sum(), len(u)
    counts[C_HIST:] = np.bincount(st, minlength=6)[:6]
    return dict(n=len(u), counts=counts, pnts=dict(u=u, v=v, idepth=idepth, iR=idepth.copy(), my_type=ty, status=st),
                kept={k: np.asarray(t[k], f32) for k in KEPT})


def set_first_stereo(orc, pyr_left, right, K4, baseline, selection_map=None, density=None, gn_mode=0):
    """selection_map None: the library's own selection on pyr_left (three levels) at `density`"""
    if selection_map is None:
        _, selection_map = select(orc, pyr_left, density)
    return set_first_with(selection_map, trace_first(orc, pyr_left[0], right, K4, baseline, gn_mode))


def from_initializer(state, keep=None):
    """STEP 3 on a state of set_first_with: keep[i] != 0 where Pnt i passed the rand() test of :1535 (None: every Pnt).  The second
    ImmaturePoint and its trace are those of setFirstStereo.  -> dict(n, counts [4], points = dict of POINT)"""
    n, K, P = state["n"], state["kept"], state["pnts"]
    kept = np.ones(n, bool) if keep is None else np.asarray(keep)[:n] != 0
    with np.errstate(invalid="ignore"):
        drop = ~np.isfinite(K["energyTH"]) | ~np.isfinite(K["idepth_min"]) | ~np.isfinite(K["idepth_max"]) | (K["idepth_min"] < 0) | (K["idepth_max"] < 0)   # :1552-1555
    made = np.nonzero(kept & ~drop)[0]
    counts = np.array([n, (~kept).sum(), (kept & drop).sum(), len(made)], np.int32)
    pts = dict(pnt=made.astype(np.int32), u=P["u"][made], v=P["v"][made], my_type=P["my_type"][made], idepth=K["idepth_stereo"][made],
               idepth_min=K["idepth_min"][made], idepth_max=K["idepth_max"][made], energyTH=K["energyTH"][made], color=K["color"][made], weights=K["weights"][made])
    return dict(n=len(made), counts=counts, points=pts)


def _bits_equal(x, y):
    if x.dtype != np.float32:
        return np.array_equal(x, y)
    return bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))


def same(a, b, keys):
    """two dicts of arrays, every float compared as bits (NaN equals NaN); returns the first member that differs, or None"""
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or not _bits_equal(x, y):
            return k
    return None
