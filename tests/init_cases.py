"""Inputs of the stereo-initialiser tests (sdso_init_*): the first stereo pair of a sequence.  synth.Scene(1001) seen from the identity pose,
the right camera at t + (-baseline, 0, 0) (immature_cases' convention), noise seeds 71 / 72, three pyramid levels for the selector."""
import functools

import numpy as np

import immature_cases as Cs
import synth

f32 = np.float32
NOISE = (71, 72)
SIZES = ((640, 480), (320, 240))
DESIRED_POINT_DENSITY = 2000.0                  # DSO's setting_desiredPointDensity; a runtime setting (the fork's default is 4000, settings.cpp:60)


def density(w, h):
    """densities[0]*w[0]*h[0] of CoarseInitializer.cpp:871 in the reference's float arithmetic"""
    return float(f32(f32(f32(0.03) * f32(w)) * f32(h)))


@functools.lru_cache(maxsize=None)
def stereo_pair(w, h):
    """dict: K4, baseline, pyr_left (3 levels of {I, dx, dy}), right (level 0), idepth (of the left camera, per pixel)"""
    cal, K4, _, _ = Cs.calib(w, h)
    T = synth.se3_exp(np.zeros(6))
    sc = synth.Scene(1001)
    left, idp = sc.render(w, h, K4, T, noise_seed=NOISE[0])
    right, _ = sc.render(w, h, K4, (T[0], T[1] + np.array([-float(cal["baseline"]), 0.0, 0.0])), noise_seed=NOISE[1])
    return dict(w=w, h=h, K4=K4, baseline=float(cal["baseline"]), pyr_left=synth.make_pyramid(left, 3), right=np.ascontiguousarray(synth.make_pyramid(right, 1)[0]),
                idepth=idp)


def keep_flags(n, seed, keep_percentage):
    """the outcome of `rand()/(float)RAND_MAX > keepPercentage` (FullSystem.cpp:1535) from a seeded generator: 1 = the Pnt goes on"""
    r = np.random.RandomState(seed).rand(n).astype(f32)
    return (~(r > f32(keep_percentage))).astype(np.uint8)


BORDER = lambda w, h: ((0, 0), (2, 100), (100, 2), (w - 4, 200), (w - 1, 50), (300, h - 4), (301, h - 1), (2, 2), (w - 4, h - 4))   # excluded
INSIDE = lambda w, h: ((3, 240, 1), (w - 5, 241, 4), (320, 3, 2), (321, h - 5, 1))                                                # just inside


@functools.lru_cache(maxsize=None)
def crafted_case():
    """On the 640 x 480 pair, in the manner of immature_cases.crafted_map_case: a map with entries 1 / 2 / 4, entries in the excluded rows
    and columns, one pixel just inside each side, and a left image with non-finite intensities under the patterns of four selected pixels
    (`bad`: their indices among the Pnts)."""
    w, h = SIZES[0]
    P = stereo_pair(w, h)
    img = P["pyr_left"][0].copy()
    m = Cs.selection_map(img, P["idepth"], 300, 9, w, h)
    for x, y in BORDER(w, h):
        m[y, x] = 2
    for x, y, t in INSIDE(w, h):
        m[y, x] = t
    inner = np.zeros((h, w), bool)
    inner[3:h - 4, 3:w - 4] = True
    ys, xs = np.nonzero(inner & (m != 0))
    bad = (10, 90, 170, 250)
    for k, v in zip(bad, (np.nan, np.inf, -np.inf, np.nan)):
        img[ys[k] + (k % 3) - 1, xs[k] + 1, 0] = v        # the pixel right of the pattern's centre row -1 / 0 / +1: read by the constructor
    return dict(P, left=img, map=m, bad=bad)


def single_entry_map(w, h):
    m = np.zeros((h, w), f32)
    m[h // 2, w // 2] = 4
    return m


def border_only_map(w, h):
    """entries, but none in the walked area"""
    m = np.zeros((h, w), f32)
    for x, y in BORDER(w, h):
        m[y, x] = 1
    return m
