"""Inputs of the full-window tests (tests/test_full_window_ref.py, tests/test_full_window_gpu.py): immature-point activation at the
window of eight keyframes that every structure is sized for — 7 residuals x 8 pattern pixels = 56 lanes of a wave in activate_point,
SDSO_IMM_MAX_HOSTS groups in ImmTraceArgs / ImmActArgs, and more selected points than the first copy back of sdso_imm_activate holds.

Three families, each built once per process (functools.lru_cache; consumers take copies, the cached arrays are never written):

  batch(name)     sdso_activate_points_batch inputs from test_stereo._activation_case at nf = 8, 7, 3, 2 with the doctoring of
                  test_stereo.test_gpu_activation_bit_exact, plus a group hosted on frame 1 whose interval is negative enough that the
                  projection into frame 0 leaves the image (frame 0 is behind frame 1, so no positive inverse depth does that): residual
                  slot 0 out of bounds.  One seed for all nf: ba_window draws frame k alike for every nf, so the smaller windows are
                  prefixes of the largest and every frame is rendered once (shared_renders).
  crafted()       nf = 3, the rule "the pixels before the first out-of-bounds pixel of a residual still add to Hdd and bd", with the
                  first failing pattern pixel chosen per point.
  resident()      seven hosts + the newest frame as a resident set with more than SDSO_IMM_ACT_FIRST_COPY selected candidates.
"""
import contextlib
import copy
import functools
import os
import re

import numpy as np

import activate_cases as AC
import distmap_cases as DC
import distmap_ref as D
import immature_cases as Cs
import immature_ref as R
import synth
import test_stereo as TS

f32 = np.float32
W, H = Cs.W, Cs.H
SEED = 3059
PATTERN = np.array([[0, -2], [-1, -1], [1, -1], [-2, 0], [0, 0], [2, 0], [-1, 1], [0, 2]], np.int32)    # patternP, as trace_dev.h / orc_stereo.cpp


def abi_define(name):
    """an integer #define of include/sdso_abi.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdso_abi.h")
    with open(path) as fh:
        return int(re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, fh.read(), re.M).group(1))


def _oracle():
    import pyoracle
    return pyoracle.load()


# ------------------------------------------------------------------ one render per view
_RENDERS = {}


@contextlib.contextmanager
def shared_renders():
    """synth.Scene.render memoised on (scene, arguments) while the block runs: the windows of one seed share their frames."""
    plain = synth.Scene.render

    def render(self, w, h, K, T_cw, noise_seed=None, aff=(0.0, 0.0), exposure=1.0):
        key = (self.planes[0][2].tobytes(), w, h, tuple(float(x) for x in K), np.asarray(T_cw[0], np.float64).tobytes(), np.asarray(T_cw[1], np.float64).tobytes(),
               noise_seed, tuple(float(x) for x in aff), float(exposure))
        if key not in _RENDERS:
            _RENDERS[key] = plain(self, w, h, K, T_cw, noise_seed=noise_seed, aff=aff, exposure=exposure)
        img, idp = _RENDERS[key]
        return img.copy(), idp.copy()

    synth.Scene.render = render
    try:
        yield
    finally:
        synth.Scene.render = plain


# ------------------------------------------------------------------ batch cases
PER_HOST = {8: 61, 7: 57, 3: 50, 2: 45}        # n = 488, 399, 150, 90: n % 4 = 0, 3, 2, 2
BATCH = {"nf8": dict(nf=8, min_obs=2), "nf8_minobs7": dict(nf=8, min_obs=7), "nf7": dict(nf=7, min_obs=2), "nf3": dict(nf=3, min_obs=2),
         "nf2": dict(nf=2, min_obs=1), "nf8_all_but_3": dict(nf=8, min_obs=2, cut=-3), "nf8_first_point": dict(nf=8, min_obs=2, cut=1)}
POINT_KEYS = ("host", "u", "v", "idepth_min", "idepth_max", "color", "weights", "energyTH", "truth")


@functools.lru_cache(maxsize=None)
def _rendered(nf):
    with shared_renders():
        return TS._activation_case(_oracle(), nf=nf, per_host=PER_HOST[nf], seed=SEED)


def undoctored(nf):
    d = _rendered(nf)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def doctor_batch(d):
    """The doctoring of test_stereo.test_gpu_activation_bit_exact, then slot 0 out of bounds for every fourth point hosted on frame 1."""
    d["idepth_max"][::17] *= 6; d["idepth_min"][5::23] *= 0.05; d["idepth_max"][5::23] *= 0.1; d["energyTH"][9::41] = np.nan
    g = np.nonzero(d["host"] == 1)[0][2::4]
    mid = np.where(np.arange(len(g)) % 2 == 0, f32(-1.0), f32(-0.7))     # 1 + t_z * idepth = 0.2 / 0.44 in frame 0: the image grows 5 / 2.3 times
    d["idepth_min"][g] = mid - f32(0.05); d["idepth_max"][g] = mid + f32(0.05)
    return d


def cut_points(d, keep):
    """the case restricted to the points `keep` (a slice or a mask)"""
    d = dict(d)
    for k in POINT_KEYS:
        d[k] = np.ascontiguousarray(d[k][keep])
    return d


def without_last_frame(d):
    """the same points without those of the last keyframe, in the window without it: (nf-1) x (nf-1) sub-tables"""
    nf = d["nf"]
    pick = [a * nf + b for a in range(nf - 1) for b in range(nf - 1)]
    out = cut_points(d, d["host"] < nf - 1)
    out.update(nf=nf - 1, pair_R=d["pair_R"][pick].copy(), pair_t=d["pair_t"][pick].copy(), pair_aff=d["pair_aff"][pick].copy())
    return out


@functools.lru_cache(maxsize=None)
def _batch(name):
    spec = BATCH[name]
    d = doctor_batch(undoctored(spec["nf"]))
    if "cut" in spec:
        d = cut_points(d, slice(None, spec["cut"]))
    return dict(d=d, min_obs=spec["min_obs"], imgs=[np.ascontiguousarray(p[0]) for p in d["win"]["pyrs"][:d["nf"]]])


def batch(name):
    return crafted() if name == "crafted" else _batch(name)


BATCH_NAMES = tuple(BATCH) + ("crafted",)


def run_oracle(orc, case, d=None, min_obs=None):
    """orc_activate_points -> (status, idepth, res_state)"""
    import ctypes as C
    from sdso_amd import abi
    d = case["d"] if d is None else d
    A, keep = TS._activate_struct(d, dI=case["imgs"][:d["nf"]], minObs=case["min_obs"] if min_obs is None else min_obs)
    n = A.n
    st, idp, rs = np.zeros(n, np.int8), np.zeros(n, f32), np.zeros((n, d["nf"]), np.uint8)
    assert orc.orc_activate_points(C.byref(A), abi.ptr(st), abi.fp(idp), abi.bp(rs)) == 0
    return st, idp, rs


def slot_states(d, res_state):
    """res_state [n, nf] by frame -> [n, nf-1] by residual slot (the r-th frame that is not the host)"""
    s = np.arange(d["nf"] - 1)[None, :]
    return np.take_along_axis(res_state, s + (s >= d["host"][:, None]), axis=1)


# ------------------------------------------------------------------ the crafted case
TX = f32(2.0)                       # the sideways pairs: t = (+-TX, 0, 0), R = I: the pattern moves by TX * fx * idepth pixels along the row
CLEARANCE = 0.3
# (first failing pattern pixel, host, how): x = the column of the pattern's centre in frame 2, y = the point's own row
CLASSES = (("right", 5, 0, 635.5), ("right", 2, 0, 636.5), ("right", 0, 0, 637.5), ("left", 3, 1, 2.6), ("left", 1, 1, 1.6), ("left", 0, 1, 0.6),
           ("bottom", 7, 0, 475.5), ("bottom", 6, 0, 476.5), ("nan", 4, 0, None))
PER_CLASS = 4


def first_failing(d, img2):
    """Per point hosted on 0 / 1 of the crafted case: the first pattern pixel of the residual into frame 2 that linearizeResidual rejects at
    the first pass (8 = none), and the smallest distance of a decision from its bound.  float32, in the operation order of activate_point."""
    fx, fy, cx, cy = [f32(x) for x in d["win"]["K"]]
    fxi, fyi = f32(1) / fx, f32(1) / fy
    nf = d["nf"]
    bad = ~np.isfinite(img2[..., 0])
    first, clear = np.full(len(d["u"]), 8, np.int32), np.full(len(d["u"]), np.inf)
    for p in range(len(d["u"])):
        pair = int(d["host"][p]) * nf + 2
        Rm, t = d["pair_R"][pair].astype(f32), d["pair_t"][pair].astype(f32)
        idepth = (d["idepth_max"][p] + d["idepth_min"][p]) * f32(0.5)
        for k in range(8):
            K0, K1, K2 = (d["u"][p] + f32(PATTERN[k, 0]) - cx) * fxi, (d["v"][p] + f32(PATTERN[k, 1]) - cy) * fyi, f32(1)
            ptp = [((Rm[3 * r] * K0 + Rm[3 * r + 1] * K1) + Rm[3 * r + 2] * K2) + t[r] * idepth for r in range(3)]
            dr = f32(1) / ptp[2]
            assert dr > 0
            Ku, Kv = (ptp[0] * dr) * fx + cx, (ptp[1] * dr) * fy + cy
            lim = (Ku - f32(1.1), Kv - f32(1.1), f32(W - 3) - Ku, f32(H - 3) - Kv)
            clear[p] = min(clear[p], min(abs(float(x)) for x in lim))
            inside = all(x > 0 for x in lim)
            if inside:
                ix, iy = int(Ku), int(Kv)
                # a non-finite intensity under or next to the four taps: which taps are read is a decision too
                if bad[max(iy - 1, 0):iy + 3, max(ix - 1, 0):ix + 3].any():
                    clear[p] = min(clear[p], float(min(Ku - ix, ix + 1 - Ku, Kv - iy, iy + 1 - Kv)))
                    inside = not bad[iy:iy + 2, ix:ix + 2].any()
            if not inside:
                first[p] = k
                break
    return first, clear


@functools.lru_cache(maxsize=1)
def _crafted():
    orc = _oracle()
    base = _rendered(3)
    win = base["win"]
    K = win["K"]
    fx, fy, cx, cy = [float(x) for x in K]
    perm = [1, 0, 2]              # frame 0 of the case is the middle keyframe: its real target, frame 1, lies behind it and sees what it sees
    nf = 3
    pick = [perm[a] * nf + perm[b] for a in range(nf) for b in range(nf)]
    pair_R, pair_t, pair_aff = base["pair_R"][pick].copy(), base["pair_t"][pick].copy(), base["pair_aff"][pick].copy()
    for host, sign in ((0, 1), (1, -1)):        # host -> frame 2: sideways, to the right for host 0 and to the left for host 1
        pair_R[host * nf + 2] = np.eye(3, dtype=f32).ravel()
        pair_t[host * nf + 2] = (sign * TX, 0, 0)
    imgs = [np.ascontiguousarray(win["pyrs"][perm[f]][0]).copy() for f in range(nf)]
    poses = [win["poses"][perm[f]] for f in range(nf)]
    with shared_renders():
        idmaps = [synth.Scene(1001).render(W, H, K, poses[f])[1] for f in range(2)]
    rs = np.random.RandomState(SEED + 1)
    hosts, us, vs, lo, hi, nan_px = [], [], [], [], [], []
    for how, _, host, target in CLASSES:
        img, idm = imgs[host], idmaps[host]
        sign = 1.0 if host == 0 else -1.0
        # the ground next to the camera is smooth: a lower gradient bar in the bottom rows (t_z of the real pair still gives Hdd >> 100)
        ok = (np.sqrt(img[..., 1] ** 2 + img[..., 2] ** 2) > (3.0 if how == "bottom" else 8.0)) & (idm > 0.0075)
        ok[:24] = False; ok[:, :24] = False; ok[:, -24:] = False
        if how != "bottom":
            ok[-24:] = False
        ys, xs = np.nonzero(ok)
        rho = idm[ys, xs].astype(np.float64)
        # the point as the other, real target sees it at its true depth: well inside
        T = synth.se3_mul(poses[1 - host], synth.se3_inv(poses[host]))
        P = (np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(len(xs))], 1) / rho[:, None]) @ T[0].T + T[1]
        pu, pv = fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy
        seen = (P[:, 2] > 0.1) & (pu > 24) & (pu < W - 24) & (pv > 24) & (pv < H - 24)
        shift = sign * float(TX) * fx * rho                                  # of the pattern in frame 2 at the true inverse depth
        if how in ("right", "left"):
            m = (target - xs) / (sign * float(TX) * fx)                      # the interval's middle that puts the centre on the target column
            cand = np.nonzero(seen & (m > 0) & (np.abs(m / rho - 1) < 0.06))[0]
            v_of = lambda i: float(ys[i])
        elif how == "bottom":
            m = rho
            cand = np.nonzero(seen & (ys == int(target)) & (xs + shift + 3 < W - 3 - 1))[0]
            v_of = lambda i: target
        else:                                                                # the centre on a half pixel of frame 2, rows on half pixels too
            m = (np.round(shift) + 0.5) / (sign * float(TX) * fx)
            cand = np.nonzero(seen & (xs + shift + 4 < W - 3 - 1) & (shift > 6))[0]
            v_of = lambda i: float(ys[i]) + 0.5
        assert len(cand) >= PER_CLASS, (how, target, len(cand))
        for i in cand[np.sort(rs.choice(len(cand), PER_CLASS, replace=False))]:
            hosts.append(host); us.append(float(xs[i])); vs.append(v_of(i))
            mid = f32(m[i])
            lo.append(mid * f32(0.9)); hi.append(mid + (mid - mid * f32(0.9)))
            if how == "nan":
                nan_px.append((int(ys[i]) + 1, int(xs[i] + np.round(shift[i])) + 1))     # under the centre's lower right tap alone
    for y, x in nan_px:
        imgs[2][y, x, 0] = np.nan
    u, v = np.array(us, f32), np.array(vs, f32)
    host = np.array(hosts, np.int32)
    color, weights, eth = np.zeros((len(u), 8), f32), np.zeros((len(u), 8), f32), np.zeros(len(u), f32)
    for h_ in (0, 1):
        s = host == h_
        c, w_, _, e = TS._oracle_init(orc, dict(w=W, h=H), imgs[h_], np.ascontiguousarray(u[s]), np.ascontiguousarray(v[s]))
        color[s], weights[s], eth[s] = c, w_, e
    d = dict(nf=nf, win=dict(K=K, pyrs=[[i] for i in imgs]), pair_R=pair_R, pair_t=pair_t, pair_aff=pair_aff, host=host, u=u, v=v, idepth_min=np.array(lo, f32),
             idepth_max=np.array(hi, f32), color=color, weights=weights, energyTH=eth, truth=np.zeros(len(u), f32))
    want = np.repeat(np.array([c[1] for c in CLASSES], np.int32), PER_CLASS)
    return dict(d=d, min_obs=1, imgs=imgs, want_first=want)


def crafted():
    """The nf = 3 window with its frames in the order (1, 0, 2), so that the real target of host 0, frame 1, lies behind it and still sees a
    point in the bottom rows.  host -> frame 2 is a pure sideways geometry (R = I, t = (+-TX, 0, 0)) for both hosts: to the right for host 0
    (the pattern leaves at w - 3: first failing pixels 5, 2, 0), to the left for host 1 (at 1.1: pixels 3, 1, 0) — one pair has one sign, and
    a positive inverse depth moves the pattern one way only.  Rows 475.5 / 476.5 of host 0 leave at h - 3 with pixels 7 / 6; the centre
    (pixel 4) fails first under one NaN intensity of frame 2 that only its lower right tap reads.  Every interval is around the true
    inverse depth, so frame 1 converges.
    -> dict(d, min_obs = 1: frame 2 is out of bounds by construction, so frame 1 is the only observation; imgs; want_first)"""
    return _crafted()


# ------------------------------------------------------------------ the resident window
XI = np.array((0.03, -0.012, 0.12, 0.002, -0.003, 0.002), np.float64)       # host k at se3_exp(k * XI), frames at k = 7, 8 (non-key) and 9 (key)
HOST_POINTS = (901, 899, 903, 897, 902, 898, 905)       # about half of a group is not activatable after three frames, and the doctoring takes 6 / 13 of the rest
NEWEST_POINTS = 97
FRAME_AFFS = ((0.02, 1.5), (0.03, 2.0), (0.01, 1.0))


@functools.lru_cache(maxsize=1)
def _resident():
    orc = _oracle()
    cal, K4, K, Ki = Cs.calib()
    sc = synth.Scene(1001)
    hosts = []
    for k, n in enumerate(HOST_POINTS):
        T = synth.se3_exp(k * XI)
        (img, idp), = Cs.images(sc, K4, T, (111 + k,))
        hosts.append(dict(T=T, img=img, map=Cs.selection_map(img, idp, n, 70 + k)))
    frames = []
    for j, aff in enumerate(FRAME_AFFS):
        T = synth.se3_exp((7 + j) * XI)
        views = Cs.images(sc, K4, T, (131 + 2 * j, 132 + 2 * j), aff=aff, baseline=cal["baseline"] if j < 2 else None)
        frames.append(dict(T=T, aff=aff, left=views[0][0], idepth=views[0][1], right=views[1][0] if j < 2 else None))
    # the eighth group is made on the last non-key frame (its geometry into the key frame is a real one) and stands for the group that the
    # newest keyframe of the window owns: activatePointsMT never walks that group, sdso_imm_trace takes it as one more named host
    newest_host = dict(T=frames[1]["T"], img=frames[1]["left"], map=Cs.selection_map(frames[1]["left"], frames[1]["idepth"], NEWEST_POINTS, 79))
    for F in frames:
        F["geom"] = [Cs.geom(K, Ki, h_["T"], F["T"], F["aff"]) for h_ in hosts + [newest_host]]
    groups = [R.add_frame(orc, h_["img"], h_["map"]) for h_ in hosts]
    for F in frames[:2]:
        R.trace(orc, [(groups[j], F["geom"][j]) for j in range(7)], F["left"], F["right"], K4, Ki.ravel(), float(cal["baseline"]))
    groups.append(R.add_frame(orc, newest_host["img"], newest_host["map"]))
    before_key = copy.deepcopy(groups)
    F = frames[2]
    key_counts, _, _ = R.trace(orc, [(groups[j], F["geom"][j]) for j in range(8)], F["left"], None, K4, Ki.ravel(), float(cal["baseline"]))
    T = [h_["T"] for h_ in hosts] + [F["T"]]
    affs = [(0.0, 0.0)] * 7 + [F["aff"]]
    nf = 8
    pair_R, pair_t, pair_aff = np.zeros((nf * nf, 9), f32), np.zeros((nf * nf, 3), f32), np.zeros((nf * nf, 2), f32)
    for h in range(nf):
        for t in range(nf):
            Rm, tv = synth.se3_mul(T[t], synth.se3_inv(T[h]))                    # leftToLeft = target.worldToCam * host.camToWorld
            pair_R[h * nf + t] = Rm.astype(f32).ravel(); pair_t[h * nf + t] = tv.astype(f32)
            a = np.exp(affs[t][0] - affs[h][0])                                  # AffLight::fromToVecExposure, exposures 1
            pair_aff[h * nf + t] = (a, affs[t][1] - a * affs[h][1])
    KRKi, Kt = DC.window_geoms(np.array([synth.se3_pack(x) for x in T]), tuple(float(x) for x in K4))
    # host 1 into the map: a pure sideways geometry as in activate_cases.window (any float values do), so that a large inverse depth leaves
    # the map; on this forward trajectory it would only approach the epipole
    fxs, fys, cxs, cys = synth.level_intrinsics(*[float(x) for x in K4], 2)
    K1 = np.array([[fxs[1], 0, cxs[1]], [0, fys[1], cys[1]], [0, 0, 1]], f32)
    K0 = np.array([[fxs[0], 0, cxs[0]], [0, fys[0], cys[0]], [0, 0, 1]], np.float64)
    KRKi[1] = K1 @ np.linalg.inv(K0).astype(f32)
    Kt[1] = np.array([0.8 * fxs[1], 0, 0], f32)
    win = dict(groups=None, imgs=[h_["img"] for h_ in hosts] + [F["left"]], flagged=np.array([1] + [0] * 7, np.uint8), KRKi=KRKi, Kt=Kt, pair_R=pair_R,
               pair_t=pair_t, pair_aff=pair_aff, K4=K4, w=W, h=H)
    S = groups[1]
    i = int(np.nonzero(np.isfinite(S["idepth_max"]) & np.isfinite(S["idepth_min"]))[0][0])       # the one seed of the map
    seeds = (np.array([1], np.int32), S["u"][i:i + 1].copy(), S["v"][i:i + 1].copy(), f32(0.5) * (S["idepth_max"][i:i + 1] + S["idepth_min"][i:i + 1]))
    return dict(win=win, before_key=before_key, after_key=groups, key_counts=key_counts, key_geom=F["geom"], K4=K4, Ki=Ki.ravel().copy(),
                baseline=float(cal["baseline"]), seeds=seeds)


def resident(doctored=True):
    """A fresh copy -> dict(win: the window of activate_ref.activate (groups = the seven walked ones + None), newest: the eighth group,
    before_key: the eight groups before the key frame's trace, key_geom, key_counts, seeds, K4, Ki, baseline, min_act_dist)"""
    c = dict(_resident())
    groups = copy.deepcopy(c.pop("after_key"))
    c["before_key"] = copy.deepcopy(c["before_key"])
    if doctored:
        for S in groups[:7]:
            AC.doctor(S)
    c["win"] = dict(c["win"], flagged=c["win"]["flagged"].copy())
    c["win"]["groups"] = groups[:7] + [None]
    c["newest"] = groups[7]
    c["min_act_dist"] = AC.MIN_ACT_DIST
    return c


def ref_map(c):
    """makeDistanceMap on the case's seeds -> the flat list that activate_ref.activate re-grows"""
    pg, u, v, idp = c["seeds"]
    _, _, m = D.make_distance_map(W, H, c["win"]["KRKi"], c["win"]["Kt"], pg, u, v, idp)
    return m
