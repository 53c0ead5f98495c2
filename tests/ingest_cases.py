"""Seeded synthetic inputs for the frame-ingest tests (raw images, response, vignette, camera models) and the helpers that drive
sdso_undistort_make_remap / sdso_ingest_* through the ctypes binding.  Nothing here is read from a dataset."""
import ctypes as C

import numpy as np

import undistort_ref as R
from sdso_amd import abi

f32, f64 = np.float32, np.float64

KITTI = dict(wOrg=1241, hOrg=376, w=1232, h=368)      # KITTI-shaped raw image and crop
VGA = dict(wOrg=640, hOrg=480, w=640, h=480)

# parsOrg per model.  KITTI-shaped: in pixels.  VGA: the "relative" format (cx, cy < 1), which readFromFile rescales (Undistort.cpp:793-809).
_PIX = [718.856, 718.856, 607.1928, 185.2157]
_REL = [0.58, 0.77, 0.5012, 0.4987]
_DIST = {
    R.PINHOLE: [0.0],
    R.FOV: [0.35],
    R.RADTAN: [-0.28, 0.07, 0.0002, 0.00002],
    R.EQUIDISTANT: [-0.05, 0.01, -0.002, 0.0005],
    R.KANNALABRANDT: [-0.04, 0.008, -0.001, 0.0002],
}
MODELS = (R.PINHOLE, R.FOV, R.RADTAN, R.EQUIDISTANT, R.KANNALABRANDT)
MODEL_NAMES = {R.PINHOLE: "Pinhole", R.FOV: "FOV", R.RADTAN: "RadTan", R.EQUIDISTANT: "Equidistant", R.KANNALABRANDT: "KannalaBrandt"}
# an explicit output K (relative fx fy cx cy, :896-909) that looks beyond the raw image: its border gets -1 entries
WIDE_K = [0.40, 0.52, 0.5, 0.5]


def pars(model, size):
    return np.array((_PIX if size is KITTI else _REL) + _DIST[model], f64)


def remap_cases():
    """(name, model, size, out_mode, out_calib): a crop for every model at both sizes, and the explicit wide K at VGA for every model."""
    out = []
    for m in MODELS:
        out.append(("%s-kitti-crop" % MODEL_NAMES[m], m, KITTI, R.CROP, None))
        out.append(("%s-vga-crop" % MODEL_NAMES[m], m, VGA, R.CROP, None))
        out.append(("%s-vga-wideK" % MODEL_NAMES[m], m, VGA, R.EXPLICIT, WIDE_K))
    return out


def raw_image(wOrg, hOrg, bits, seed):
    """A smooth pattern with texture and noise over the full range of the pixel type."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:hOrg, 0:wOrg].astype(f64)
    top = float((1 << bits) - 1)
    v = 0.5 + 0.22 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0) + 0.18 * np.sin((x + 2 * y) / 5.0) + 0.1 * rs.normal(0, 1, (hOrg, wOrg))
    return np.clip(v * top, 0, top).astype(np.uint8 if bits == 8 else np.uint16)


def response(bits):
    """A strictly increasing G as PhotometricUndistorter holds it after :114-123 (0 .. 255)."""
    n = 1 << bits
    t = np.arange(n, dtype=f64) / (n - 1)
    g = (0.7 * t + 0.3 * t ** 2.2)
    G = (255.0 * (g - g[0]) / (g[-1] - g[0])).astype(f32)
    assert (np.diff(G) > 0).all()
    return G


def vignette_inv(wOrg, hOrg):
    """1 / vignetteMap (:179-181) of a smooth fall-off towards the corners."""
    y, x = np.mgrid[0:hOrg, 0:wOrg].astype(f64)
    r2 = ((x - 0.52 * wOrg) / wOrg) ** 2 + ((y - 0.47 * hOrg) / hOrg) ** 2
    vm = (1.0 - 0.9 * r2).astype(f32)
    return (f32(1.0) / (vm / vm.max())).astype(f32)


# ------------------------------------------------------------------ the library through ctypes
def lib_make_remap(model, parsOrg, size, out_mode, out_calib=None):
    """sdso_undistort_make_remap: (rc, K, remapX, remapY, passthrough)."""
    L = abi.load()
    w, h = size["w"], size["h"]
    K = np.zeros(4, f64)
    rx, ry = np.zeros((h, w), f32), np.zeros((h, w), f32)
    pt = C.c_int(-1)
    p = np.ascontiguousarray(parsOrg, f64)
    oc = np.ascontiguousarray(out_calib, f32) if out_calib is not None else None
    rc = L.sdso_undistort_make_remap(model, abi.dp(p), size["wOrg"], size["hOrg"], w, h, out_mode, abi.fp(oc) if oc is not None else None,
                                     abi.dp(K), abi.fp(rx), abi.fp(ry), C.byref(pt))
    return rc, K, rx, ry, pt.value


def calib_create(ctx, calib, size, remap, bits, G, vinv, mode, use_exposure=True):
    """sdso_ingest_calib_create; remap = (remapX, remapY) or None for passthrough.  Returns the rc."""
    rx = np.ascontiguousarray(remap[0], f32) if remap is not None else None
    ry = np.ascontiguousarray(remap[1], f32) if remap is not None else None
    Gc = np.ascontiguousarray(G, f32) if G is not None else None
    vc = np.ascontiguousarray(vinv, f32) if vinv is not None else None
    nul = None
    return ctx.L.sdso_ingest_calib_create(ctx.h, calib, size["wOrg"], size["hOrg"], size["w"], size["h"], abi.fp(rx) if rx is not None else nul,
                                          abi.fp(ry) if ry is not None else nul, bits // 8, abi.fp(Gc) if Gc is not None else nul,
                                          abi.fp(vc) if vc is not None else nul, mode, 1 if use_exposure else 0)


def download_pyramid(ctx, slot, w, h):
    """Every level of a slot: list of (dI (h_l, w_l, 3), absSquaredGrad (h_l, w_l))."""
    out = []
    for lvl in range(ctx.L.sdso_pyramid_levels(w, h)):
        wl, hl = w >> lvl, h >> lvl
        dI, ag = np.zeros((hl, wl, 3), f32), np.zeros((hl, wl), f32)
        ctx.check(ctx.L.sdso_download_pyramid_level(ctx.h, slot, lvl, abi.fp(dI)))
        ctx.check(ctx.L.sdso_download_abs_grad(ctx.h, slot, lvl, abi.fp(ag)))
        out.append((dI, ag))
    return out


def make_pyramid(ctx, slot, img):
    img = np.ascontiguousarray(img, f32)
    ctx.check(ctx.L.sdso_make_pyramid(ctx.h, slot, img.shape[1], img.shape[0], abi.fp(img)))


def same_bits(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(a, b)) and len(a) == len(b)
