"""Inputs of the stereoMatch tests, from tests/immature_cases.py: the stereo pair of frame 0 of window_case() (640 x 480, synth.Scene(1001))
and selection maps of 1037, 259, 1 and 0 points on its left image."""
import functools

import numpy as np

import immature_cases as Cs
import synth

POINTS = (1037, 259, 1, 0)
SEED = 5


@functools.lru_cache(maxsize=1)
def pair():
    cal, K4, K, Ki = Cs.calib()
    T = synth.se3_exp(np.array(Cs.MOTIONS[0], np.float64))
    (left, idp), (right, _) = Cs.images(synth.Scene(1001), K4, T, Cs.NOISE[0], aff=Cs.AFFS[0], baseline=cal["baseline"])
    maps = {n: Cs.selection_map(left, idp, n, SEED) for n in POINTS}
    return dict(K4=K4, baseline=float(cal["baseline"]), left=left, right=right, maps=maps)


@functools.lru_cache(maxsize=1)
def other_host():
    """Host 1 of window_case() with its 259 points and its geometry into the pair's left frame: a group for sdso_imm_trace next to the
    one stereoMatch walks."""
    cal, K4, K, Ki = Cs.calib()
    T_host = synth.se3_exp(np.array(Cs.HOST_POSES[1], np.float64))
    (img, idp), = Cs.images(synth.Scene(1001), K4, T_host, (12,))
    g = Cs.geom(K, Ki, T_host, synth.se3_exp(np.array(Cs.MOTIONS[0], np.float64)), Cs.AFFS[0])
    return dict(img=img, map=Cs.selection_map(img, idp, 259, Cs.HOST_SEEDS[1]), geom=g, Ki=Ki.ravel().copy())
