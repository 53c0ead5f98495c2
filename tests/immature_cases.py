"""Inputs of the immature-point tests: one 640x480 scene (synth.Scene), hosts at different poses, successive stereo frames.

The right camera of a frame is its left pose with t + (-baseline, 0, 0), as in synth.stereo_problem."""
import numpy as np

import synth

f32 = np.float32
W, H = 640, 480
HOST_POINTS = (1037, 259, 1)                # not multiples of 4, 16, 64 or 256; a fourth host comes from an all-zero map
HOST_POSES = ((0, 0, 0, 0, 0, 0), (0.05, -0.02, 0.30, 0.004, -0.006, 0.005), (-0.04, 0.01, 0.15, -0.003, 0.004, -0.002))
HOST_SEEDS = (5, 6, 7)
# world (= host 0) -> frame
MOTIONS = ((0.25, -0.06, 0.10, 0.006, -0.01, 0.012), (0.35, -0.08, 0.45, 0.008, -0.012, 0.015), (0.40, -0.08, 0.90, 0.008, -0.014, 0.017),
           (0.42, -0.09, 1.10, 0.009, -0.014, 0.018))
AFFS = ((0.02, 1.5), (0.03, 2.0), (0.01, 1.0), (0.0, 0.5))
NOISE = ((21, 22), (31, 32), (41, 42), (51, 52))


def calib(w=W, h=H):
    cal = synth.kitti_calib(w, h)
    K4 = np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"]], f32)
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], f32)
    Ki = np.linalg.inv(K.astype(np.float64)).astype(f32)            # the caller's K.inverse()
    return cal, K4, K, Ki


def geom(K, Ki, T_host, T_frame, aff_frame):
    """What the caller computes at FullSystem.cpp:654-665 (host affine (0, 0), exposures 1)."""
    R, t = synth.se3_mul(T_frame, synth.se3_inv(T_host))              # hostToNew
    R, t = R.astype(f32), t.astype(f32)
    a = f32(np.exp(aff_frame[0]))
    return dict(KRKi=(K @ R @ Ki).astype(f32).ravel(), Kt=(K @ t).astype(f32), aff=np.array([a, aff_frame[1]], f32),
                KRi=(K @ R.T).astype(f32).ravel(), t=t)


def images(scene, K4, T, noise, aff=(0.0, 0.0), baseline=None, w=W, h=H):
    """level-0 {I, dx, dy} of the left camera at world-to-camera T and, with a baseline, of the right one"""
    out = []
    for k, Tc in enumerate([T] if baseline is None else [T, (T[0], T[1] + np.array([-float(baseline), 0.0, 0.0]))]):
        img, idepth = scene.render(w, h, K4, Tc, noise_seed=noise[k], aff=aff)
        out.append((np.ascontiguousarray(synth.make_pyramid(img, 1)[0]), idepth))
    return out


def selection_map(dI0, idepth, n, seed, w=W, h=H):
    """n selected pixels with types 1 / 2 / 4 in turn (a PixelSelector map), away from the border"""
    m = np.zeros((h, w), f32)
    if n:
        u, v = synth.select_points(dI0, n, seed, idepth=idepth, min_idepth=0.0075)
        m[v, u] = np.array([1, 2, 4], f32)[np.arange(n) % 3]
    return m


def window_case():
    """Three hosts (+ one without points) and four stereo frames."""
    cal, K4, K, Ki = calib()
    sc = synth.Scene(1001)
    hosts = []
    for k, (xi, n) in enumerate(zip(HOST_POSES, HOST_POINTS)):
        T = synth.se3_exp(np.array(xi, np.float64))
        (img, idp), = images(sc, K4, T, (11 + k,))
        hosts.append(dict(T=T, img=img, map=selection_map(img, idp, n, HOST_SEEDS[k])))
    hosts.append(dict(T=hosts[0]["T"], img=hosts[0]["img"], map=np.zeros((H, W), f32)))
    frames = []
    for xi, aff, noise in zip(MOTIONS, AFFS, NOISE):
        T = synth.se3_exp(np.array(xi, np.float64))
        (left, _), (right, _) = images(sc, K4, T, noise, aff=aff, baseline=cal["baseline"])
        frames.append(dict(T=T, aff=aff, left=left, right=right, geom=[geom(K, Ki, h_["T"], T, aff) for h_ in hosts]))
    return dict(K4=K4, Ki=Ki.ravel().copy(), baseline=float(cal["baseline"]), hosts=hosts, frames=frames)


def crafted_map_case():
    """A map with entries 1, 2 and 4, entries in the excluded border rows and columns (x, y < 3, x >= w-4, y >= h-4), one pixel just inside
    on every side, and an image with a handful of non-finite intensities under selected patterns."""
    cal, K4, K, Ki = calib()
    (img, idp), = images(synth.Scene(1001), K4, synth.se3_exp(np.zeros(6)), (61,))
    m = selection_map(img, idp, 300, 9)
    for x, y in ((0, 0), (2, 100), (100, 2), (W - 4, 200), (W - 1, 50), (300, H - 4), (301, H - 1), (2, 2), (W - 4, H - 4)):   # excluded
        m[y, x] = 2
    for x, y, t in ((3, 240, 1), (W - 5, 241, 4), (320, 3, 2), (321, H - 5, 1)):                                                            # just inside
        m[y, x] = t
    ys, xs = np.nonzero(m)
    img = img.copy()
    for k, bad in zip((10, 90, 170, 250), (np.nan, np.inf, -np.inf, np.nan)):     # under the pattern of four selected pixels
        img[ys[k] + (k % 3) - 1, xs[k] + 1, 0] = bad
    return dict(img=img, map=m)
