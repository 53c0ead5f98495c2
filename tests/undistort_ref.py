"""CPU statement of the reference's Undistort (geometry + photometric step), for the tests.

Written from the behaviour of the reference (paths under src/util):
  PhotometricUndistorter::processFrame   Undistort.cpp:222-260    (factor * raw | G[raw] | G[raw] * vignetteMapInv; the exposure rule)
  Undistort::undistort<T>                Undistort.cpp:398-489    (steps 1 and 2; the benchmark noise and applyBlurNoise are zero by default)
  Undistort::makeOptimalK_crop           Undistort.cpp:586-709
  Undistort::readFromFile                Undistort.cpp:793-949    (relative-format rescale, output K, remap loop with its fix-ups)
  Undistort*::distortCoordinates         Undistort.cpp:974-1236   (FOV, RadTan, Equidistant, KannalaBrandt, Pinhole)
Arithmetic is NumPy float32, one rounding per operation, left to right; where the reference mixes double and float (the 2.0 literals of
RadTan at :1060-1061, the Mat33 K, `*= 1.01`) the C promotion rules are followed with explicit float64 steps.  `trans` selects how the
transcendental calls (tan / atan / atan2) are evaluated: "f32" in float32, "f64" in float64 rounded to float32 — the two differ by what a
libm may differ from NumPy, which is how the tests bound the comparison for the three models that use them.
"""
import numpy as np

f32, f64 = np.float32, np.float64
PINHOLE, FOV, RADTAN, EQUIDISTANT, KANNALABRANDT = range(5)
CROP, NONE, FULL, EXPLICIT = range(4)
NPARS = {PINHOLE: 5, FOV: 5, RADTAN: 8, EQUIDISTANT: 8, KANNALABRANDT: 8}


class UndistortError(ValueError):
    """The reference exits or asserts here; the library returns SDSO_ERR_ARG."""


def _t(fn, trans, *a):
    if trans == "f32":
        return fn(*[np.asarray(x, f32) for x in a]).astype(f32)
    return fn(*[np.asarray(x, f64) for x in a]).astype(f32)


def distort(model, pars, K, x, y, trans="f32"):
    """distortCoordinates of `model` on float32 arrays x, y; pars = parsOrg (float64, pixels), K = (fx fy cx cy) of the Mat33 (float64)."""
    p = [f32(v) for v in list(pars) + [0.0] * (8 - len(pars))]        # `float fx = parsOrg[0]` ...
    fx, fy, cx, cy = p[:4]
    ofx, ofy, ocx, ocy = [f32(v) for v in K]
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    one = f32(1)
    with np.errstate(all="ignore"):
        ix = (x - ocx) / ofx
        iy = (y - ocy) / ofy
        if model == PINHOLE:                                             # :1229-1232
            return fx * ix + cx, fy * iy + cy
        if model == FOV:                                                 # :976-1003
            dist = p[4]
            d2t = f32(2) * _t(np.tan, trans, dist / f32(2))
            r = np.sqrt(ix * ix + iy * iy)
            fac = _t(np.arctan, trans, r * d2t) / (dist * r)
            fac = np.where((r == 0) | (dist == 0), one, fac).astype(f32)
            return fx * fac * ix + cx, fy * fac * iy + cy
        if model == RADTAN:                                              # :1053-1063
            k1, k2, r1, r2 = p[4:8]
            mx2, my2, mxy = ix * ix, iy * iy, ix * iy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            two = f64(2.0)
            xd = ((ix + ix * rad).astype(f64) + two * f64(r1) * mxy.astype(f64)) + f64(r2) * (rho2.astype(f64) + two * mx2.astype(f64))
            yd = ((iy + iy * rad).astype(f64) + two * f64(r2) * mxy.astype(f64)) + f64(r1) * (rho2.astype(f64) + two * my2.astype(f64))
            return fx * xd.astype(f32) + cx, fy * yd.astype(f32) + cy
        if model == EQUIDISTANT:                                         # :1114-1125
            k1, k2, k3, k4 = p[4:8]
            r = np.sqrt(ix * ix + iy * iy)
            th = _t(np.arctan, trans, r)
            th2 = th * th
            th4 = th2 * th2
            th6 = th4 * th2
            th8 = th4 * th4
            thd = th * (one + k1 * th2 + k2 * th4 + k3 * th6 + k4 * th8)
            scaling = np.where(r.astype(f64) > 1e-8, thd / r, one).astype(f32)
            return fx * ix * scaling + cx, fy * iy * scaling + cy
        if model == KANNALABRANDT:                                       # :1170-1192
            k0, k1, k2, k3 = p[4:8]
            s = np.sqrt(ix * ix + iy * iy)
            th = _t(np.arctan2, trans, s, np.ones_like(s))
            th2 = th * th
            th3 = th2 * th
            th5 = th3 * th2
            th7 = th5 * th2
            th9 = th7 * th2
            r = th + k0 * th3 + k1 * th5 + k2 * th7 + k3 * th9
            q = r / s
            ox = np.where(s.astype(f64) < 1e-6, fx * ix + cx, q * fx * ix + cx).astype(f32)
            oy = np.where(s.astype(f64) < 1e-6, fy * iy + cy, q * fy * iy + cy).astype(f32)
            return ox, oy
    raise UndistortError("unknown model")


def make_optimal_k_crop(model, pars, wOrg, hOrg, w, h, trans="f32"):
    """makeOptimalK_crop (:586-709): K as four float64 (the Mat33 entries), or UndistortError after 500 shrink steps (:698-701)."""
    ident = (1.0, 1.0, 0.0, 0.0)                                         # K.setIdentity(), :588
    t = ((np.arange(100000) - f32(50000.0)).astype(f32) / f32(10000.0)).astype(f32)
    zero = np.zeros(100000, f32)

    def span(vals, lim):
        ok = np.nonzero((vals > 0) & (vals < f32(lim - 1)))[0]
        if len(ok) == 0:
            return f32(0), f32(0)
        nz = ok[t[ok] != 0]                                              # `if(minX==0) minX = ...` keeps re-assigning while it is 0
        return (t[nz[0]] if len(nz) else f32(0)), t[ok[-1]]

    gx, _ = distort(model, pars, ident, t, zero, trans)
    minX, maxX = span(gx, wOrg)
    _, gy = distort(model, pars, ident, zero, t, trans)
    minY, maxY = span(gy, hOrg)
    minX, maxX, minY, maxY = [f32(f64(v) * 1.01) for v in (minX, maxX, minY, maxY)]     # :626-629, float *= double

    ys = np.arange(h).astype(f32)
    xs = np.arange(w).astype(f32)
    iteration = 0
    while True:
        ry = np.repeat(minY + (maxY - minY) * ys / (f32(h) - f32(1.0)), 2).astype(f32)
        rx = np.tile(np.array([minX, maxX], f32), h)
        dx, _ = distort(model, pars, ident, rx, ry, trans)
        with np.errstate(invalid="ignore"):
            inside = (dx > 0) & (dx < f32(wOrg - 1))
        oobLeft, oobRight = bool((~inside[0::2]).any()), bool((~inside[1::2]).any())
        rx = np.repeat(minX + (maxX - minX) * xs / (f32(w) - f32(1.0)), 2).astype(f32)
        ry = np.tile(np.array([minY, maxY], f32), w)
        _, dy = distort(model, pars, ident, rx, ry, trans)
        with np.errstate(invalid="ignore"):
            inside = (dy > 0) & (dy < f32(hOrg - 1))
        oobTop, oobBottom = bool((~inside[0::2]).any()), bool((~inside[1::2]).any())
        again = oobLeft or oobRight or oobTop or oobBottom
        if (oobLeft or oobRight) and (oobTop or oobBottom):
            if (maxX - minX) > (maxY - minY):
                oobBottom = oobTop = False
            else:
                oobLeft = oobRight = False
        if oobLeft:
            minX = f32(f64(minX) * 0.995)
        if oobRight:
            maxX = f32(f64(maxX) * 0.995)
        if oobTop:
            minY = f32(f64(minY) * 0.995)
        if oobBottom:
            maxY = f32(f64(maxY) * 0.995)
        iteration += 1
        if iteration > 500:                                                # :698-701, tested before the loop condition
            raise UndistortError("makeOptimalK_crop does not converge")
        if not again:
            break
    with np.errstate(all="ignore"):
        k00 = f64((f32(w) - f32(1.0)) / (maxX - minX))
        k11 = f64((f32(h) - f32(1.0)) / (maxY - minY))
    return np.array([k00, k11, f64(-minX) * k00, f64(-minY) * k11], f64)   # :705-708, the products are double


def make_remap(model, parsOrg, wOrg, hOrg, w, h, out_mode, out_calib=None, trans="f32", with_coords=False):
    """readFromFile behind its parsing (:793-949).  Returns (K float64[4], remapX, remapY float32 (h, w), passthrough); with_coords adds
    the coordinates (ix, iy) the validity test of :939 saw."""
    pars = np.array(parsOrg, f64)[:NPARS[model]].copy()
    if pars[2] < 1 and pars[3] < 1:                                       # :793-809
        pars[0] = pars[0] * wOrg
        pars[1] = pars[1] * hOrg
        pars[2] = pars[2] * wOrg - 0.5
        pars[3] = pars[3] * hOrg - 0.5
    passthrough = False
    if out_mode == CROP:
        K = make_optimal_k_crop(model, pars, wOrg, hOrg, w, h, trans)
    elif out_mode == NONE:                                                # :882-895
        if w != wOrg or h != hOrg:
            raise UndistortError("rectification mode none requires input and output dimensions to match")
        K = pars[:4].copy()
        passthrough = True
    elif out_mode == EXPLICIT:                                            # :896-909: float * int is float, `- 0.5` makes it double
        oc = np.asarray(out_calib, f32)
        K = np.array([f64(oc[0] * f32(w)), f64(oc[1] * f32(h)), f64(oc[2] * f32(w)) - 0.5, f64(oc[3] * f32(h)) - 0.5], f64)
    else:                                                                 # makeOptimalK_full: assert(false), :711-714
        raise UndistortError("makeOptimalK_full is not implemented in the reference")
    gx, gy = np.meshgrid(np.arange(w).astype(f32), np.arange(h).astype(f32))
    ix, iy = distort(model, pars, K, gx.ravel(), gy.ravel(), trans)
    ix, iy = ix.astype(f32).copy(), iy.astype(f32).copy()
    # :934-937 in order; the last line writes ix (sic)
    ix[ix == 0] = f32(0.001)
    iy[iy == 0] = f32(0.001)
    ix[ix == f32(wOrg - 1)] = f32(wOrg - 1.001)
    ix[iy == f32(hOrg - 1)] = f32(hOrg - 1.001)
    with np.errstate(invalid="ignore"):
        ok = (ix > 0) & (iy > 0) & (ix < f32(wOrg - 1)) & (iy < f32(wOrg - 1))   # :939, iy against wOrg (sic)
    rx = np.where(ok, ix, f32(-1)).astype(f32).reshape(h, w)
    ry = np.where(ok, iy, f32(-1)).astype(f32).reshape(h, w)
    if with_coords:
        return K, rx, ry, passthrough, ix.reshape(h, w), iy.reshape(h, w)
    return K, rx, ry, passthrough


def sanitize_remap(remapX, remapY, wOrg, hOrg):
    """What sdso_ingest_calib_create does to caller-owned tables: an entry with remapX >= 0 whose four taps (int)x, (int)y, +1, +1 do not
    all lie inside wOrg x hOrg — an out-of-bounds read in the reference — becomes "outside" (-1, -1).  Everything else is kept."""
    x, y = np.asarray(remapX, f32), np.asarray(remapY, f32)
    with np.errstate(invalid="ignore"):
        inside = (x >= 0) & (x < f32(wOrg - 1)) & (y > f32(-1)) & (y < f32(hOrg - 1))
    return np.where(inside, x, f32(-1)).astype(f32), np.where(inside, y, f32(-1)).astype(f32)


def process_frame(raw, G, vinv, mode, exposure, factor, use_exposure=True):
    """PhotometricUndistorter::processFrame (:222-260): (float32 image, output exposure_time).  G None = !valid."""
    raw = np.asarray(raw)
    if G is None or exposure <= 0 or mode == 0:                           # :231
        img = f32(factor) * raw.astype(f32)
    else:
        img = np.asarray(G, f32)[raw.astype(np.int64)]
        if mode == 2:
            img = img * np.asarray(vinv, f32).reshape(raw.shape)
    return img.astype(f32), (f32(exposure) if use_exposure else f32(1))   # :253-259


def remap_image(img, remapX, remapY):
    """Step 2 of Undistort::undistort (:433-474) without the benchmark noise: bilinear remap in the summation order of :469-472."""
    hOrg, wOrg = img.shape
    src = np.asarray(img, f32).ravel()
    xx, yy = np.asarray(remapX, f32).ravel().copy(), np.asarray(remapY, f32).ravel().copy()
    out = np.zeros(xx.shape, f32)                                          # xx < 0 -> 0, :454-456
    m = ~(xx < 0)
    x, y = xx[m], yy[m]
    xi, yi = x.astype(np.int64), y.astype(np.int64)                         # C conversion: truncation toward zero
    x = x - xi.astype(f32)
    y = y - yi.astype(f32)
    xy = x * y
    b = xi + yi * wOrg
    if ((xi < 0) | (xi > wOrg - 2) | (yi < 0) | (yi > hOrg - 2)).any():
        raise UndistortError("a tap lies outside the raw image: the reference reads out of bounds here (see sanitize_remap)")
    out[m] = xy * src[b + 1 + wOrg] + (y - xy) * src[b + wOrg] + (x - xy) * src[b + 1] + (f32(1) - x - y + xy) * src[b]
    return out.reshape(np.asarray(remapX).shape)


def undistort(raw, remapX, remapY, G, vinv, mode, exposure, factor=1.0, use_exposure=True):
    """Undistort::undistort<T> (:398-489): (float32 w x h image, exposure).  remapX None = passthrough (:481-483)."""
    img, ex = process_frame(raw, G, vinv, mode, exposure, factor, use_exposure)
    if remapX is None:
        return img.copy(), ex
    return remap_image(img, remapX, remapY), ex
