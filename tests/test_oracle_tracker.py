"""CPU-only checks of the oracle's tracker restatement (parity unpinned by reference fixtures:
the reference has none for this path).  Independent evidence used instead:
  * the 8 Jacobian columns accumulated into b = J^T W r agree with a finite-difference derivative
    of the Huber energy w.r.t. the left-multiplied increment (double re-evaluation);
  * the DSO-native LM recovers the synthetic motion;
  * the pyramid rule of the generator equals the oracle's makeImages restatement bit-for-bit.

makeCoarseDepthL0 STEP1-splat .. STEP5 (CoarseTracker.cpp:352-534) has two float restatements: the oracle's orc_make_coarse_depth
and the numpy synth.make_pc.  They must agree bit for bit at window scale (1232x368 and 640x480, up to 20 000 points, pixels shared
across the 2048-point tiles of the device splat), and both are held to coarse_depth_truth, a float64 truth that does not depend on
summation order.  With positive idepths and weights the kept pixels and their order equal the truth's; the normalised idepth's
largest relative error to the truth, measured on the CPU over three seeds each of n = 1, 257, 2049, 4097, 20 000 and over 4000
selected points of a rendered scene, both shapes:
  level           0        1        2        3        4
  measured     2.9e-7   2.9e-7   4.1e-7   3.1e-7   3.3e-7
  bar          9e-7     9e-7     1.2e-6   1e-6     1e-6
The device path (sdso_track_make_ref) is bit-identical to both restatements (tests/test_tracking_ref_gpu.py), so these bars are its
bars too."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth


@pytest.fixture(scope="module")
def prob():
    return synth.tracker_problem(w=640, h=480, npts=2000, seed=2001)


def test_pyramid_rule_matches_oracle(oracle, prob):
    img = np.ascontiguousarray(prob["pyr_new"][0][..., 0])
    h, w = img.shape
    L = oracle.orc_pyramid_levels(w, h)
    assert L == prob["levels"] == synth.pyramid_levels(w, h)
    outs = [np.zeros(((h >> l), (w >> l), 3), np.float32) for l in range(L)]
    ptrs = (abi.c_float_p * L)(*[abi.fp(o) for o in outs])
    oracle.orc_make_images(abi.fp(img), w, h, L, ptrs)
    for l in range(L):
        assert np.array_equal(outs[l], prob["pyr_new"][l])


def test_pyramid_level_rule(oracle):
    assert oracle.orc_pyramid_levels(1241, 376) == 1          # odd width: no coarser level (globalCalib.cpp:52-58)
    assert oracle.orc_pyramid_levels(1232, 368) == 5
    assert oracle.orc_pyramid_levels(640, 480) == 4


def _energy_double(prob, lvl, T, aff, prm):
    """Huber energy of calcRes in double, fixed inlier set irrelevant: sum over in-bounds points."""
    pc = prob["pc"][lvl]
    img = prob["pyr_new"][lvl].astype(np.float64)
    h, w, _ = img.shape
    fx, fy, cx, cy = [float(prob[k][lvl]) for k in ("fx", "fy", "cx", "cy")]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    R, t = T
    x, y, idp, col = [pc[k].astype(np.float64) for k in ("u", "v", "idepth", "color")]
    P = (R @ np.linalg.inv(K) @ np.stack([x, y, np.ones_like(x)])) + t[:, None] * idp[None, :]
    u, v = P[0] / P[2], P[1] / P[2]
    Ku, Kv = fx * u + cx, fy * v + cy
    ok = (Ku > 2) & (Kv > 2) & (Ku < w - 3) & (Kv < h - 3) & (idp / P[2] > 0)
    Ku, Kv, col = Ku[ok], Kv[ok], col[ok]
    ix, iy = Ku.astype(int), Kv.astype(int)
    dx, dy = Ku - ix, Kv - iy
    I = (dx * dy * img[iy + 1, ix + 1, 0] + (dy - dx * dy) * img[iy + 1, ix, 0] + (dx - dx * dy) * img[iy, ix + 1, 0]
         + (1 - dx - dy + dx * dy) * img[iy, ix, 0])
    a = np.exp(aff[0] - 0.0)
    r = I - (a * col + (aff[1] - a * 0.0))
    ar = np.abs(r)
    e = np.where(ar < 9, r * r, 9 * (2 * ar - 9))       # hw*r^2*(2-hw)
    return e.sum(), len(r)


def _smooth_problem():
    """A smooth image (wavelength >= 40 px, no edges, no noise) and arbitrary template points: the
    Jacobian check needs no photo-consistency, only that the stored central-difference gradient
    equals the derivative of the bilinear interpolant to a few per cent."""
    w, h = 320, 240
    rs = np.random.RandomState(77)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = np.full((h, w), 120.0)
    for _ in range(12):
        lam = rs.uniform(40, 160)
        ang = rs.uniform(0, 2 * np.pi)
        img += rs.uniform(4, 10) * np.sin(2 * np.pi / lam * (np.cos(ang) * xs + np.sin(ang) * ys) + rs.uniform(0, 6.28))
    pyr = synth.make_pyramid(img.astype(np.float32), levels=2)
    n = 3000
    u = rs.randint(8, w // 2 - 8, n).astype(np.float32)
    v = rs.randint(8, h // 2 - 8, n).astype(np.float32)
    pc1 = dict(u=u, v=v, idepth=rs.uniform(0.02, 0.2, n).astype(np.float32),
               color=(pyr[1][v.astype(int), u.astype(int), 0] + rs.normal(0, 6, n)).astype(np.float32))
    cal = synth.kitti_calib(w, h)
    fxs, fys, cxs, cys = synth.level_intrinsics(cal["fx"], cal["fy"], cal["cx"], cal["cy"], 2)
    return dict(levels=2, pyr_ref=pyr, pyr_new=pyr, pc=[pc1, pc1], fx=fxs, fy=fys, cx=cxs, cy=cys)


def test_b_is_energy_gradient(oracle):
    prob = _smooth_problem()
    lvl = 1
    prm = helpers.track_params(prob)
    T0 = synth.se3_exp(np.array([0.015, -0.008, 0.3, 0.003, -0.005, 0.0015]))
    aff0 = (0.01, 1.0)
    ev = abi.TrackEval()
    oracle.orc_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T0)), C.byref(abi.Aff(*aff0)), 10.0, C.byref(ev))
    H, b, res, nw, mask = helpers.oracle_eval(oracle, prob["pc"][lvl], prob["pyr_new"][lvl], ev)
    assert res[5] == 0 and (int(mask.sum()) + 3) // 4 * 4 == nw      # cutoff 200: nothing saturated
    n = nw
    # b is scaled by [ROT,ROT,ROT,TRANS,TRANS,TRANS,A,B] (the reference's swapped order, CoarseTracker.cpp:584-595)
    SC = np.array([1, 1, 1, 0.5, 0.5, 0.5, 10, 1000.0])
    g = np.zeros(8)
    for k in range(8):
        eps = 1e-6
        d = np.zeros(8)
        d[k] = eps
        Tp = synth.se3_mul(synth.se3_exp(d[:6]), T0)
        Tm = synth.se3_mul(synth.se3_exp(-d[:6]), T0)
        ep, _ = _energy_double(prob, lvl, Tp, (aff0[0] + d[6], aff0[1] + d[7]), prm)
        em, _ = _energy_double(prob, lvl, Tm, (aff0[0] - d[6], aff0[1] - d[7]), prm)
        g[k] = (ep - em) / (2 * eps) / 2.0 / n            # dE/dx / 2 = J^T w r ; /n as calcGSSSE :581-582
    # bilinear interpolation makes E piecewise smooth; the analytic J uses the interpolated image
    # gradient instead of the exact derivative of the interpolant, so agreement is approximate.
    assert np.allclose(b / SC, g, rtol=0.03, atol=2e-3 * np.abs(g).max())


def test_lm_recovers_motion(oracle, prob):
    prm = helpers.track_params(prob)
    T, aff, out = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    assert out.good == 1
    R, t = T.Rt()
    Rt, tt = prob["refToNew_true"]
    assert np.abs(t - tt).max() < 5e-3
    assert np.abs(R - Rt).max() < 1e-3
    assert out.lastResiduals[0] < 8.0
    assert out.evaluations >= 8 and out.point_evals > 0


def test_abort_on_min_res(oracle, prob):
    prm = helpers.track_params(prob)
    for i in range(5):
        prm.minResForAbort[i] = 0.01      # every level is "worse than achieved" -> abort at the coarsest level
    T, aff, out = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    assert out.good == 0
    assert np.isnan(out.lastResiduals[0]) and not np.isnan(out.lastResiduals[prob["levels"] - 1])
    assert np.array_equal(T.Rt()[0], np.eye(3))           # outputs untouched on abort (CoarseTracker.cpp:1032-1047)


def test_make_coarse_depth_oracle_equals_the_generator(oracle):
    """makeCoarseDepthL0 STEP1-splat .. STEP5 (CoarseTracker.cpp:352-534): the oracle's C++ restatement (the checker of the device
    kernels) and the numpy generator behind every synthetic tracking problem (sdso_amd/synth.py::make_pc) are two independent
    restatements of the same loops — identical pc_n, order and floats, including pixels hit by several points and weights != 1."""
    import pyoracle
    import synth
    prob = synth.tracker_problem(w=320, h=240, npts=500, seed=2107)
    u, v, idp = prob["points"]
    rs = np.random.RandomState(8)
    u = u.astype(np.int32).copy(); v = v.astype(np.int32).copy()
    for dst, src in ((10, 400), (11, 400), (12, 400), (20, 300), (450, 3)):
        u[dst], v[dst] = u[src], v[src]
    wgt = rs.uniform(0.2, 3.0, len(u)).astype(np.float32)
    idp = (idp * rs.uniform(0.9, 1.1, len(u))).astype(np.float32)
    a = synth.make_pc(u, v, idp, wgt, prob["pyr_ref"])
    b = pyoracle.make_coarse_depth(oracle, u, v, idp, wgt, prob["pyr_ref"])
    assert len(a) == len(b) == prob["levels"]
    for l in range(prob["levels"]):
        assert len(a[l]["u"]) == len(b[l]["u"]) > 0
        for k in ("u", "v", "idepth", "color"):
            assert np.array_equal(a[l][k], b[l][k]), (l, k)


# ------------------------------------------------------------------ makeCoarseDepthL0 at window scale
CD_BARS = (9e-7, 9e-7, 1.2e-6, 1e-6, 1e-6)      # per level: about 3x the largest error measured (module docstring)


def coarse_depth_truth(u, v, idp, wgt, ref_pyr):
    """makeCoarseDepthL0 STEP1-splat .. STEP5 (CoarseTracker.cpp:352-534) in float64, written so that no result depends on the order of
    a sum: the splat is np.bincount, the pyramid 2x2 block sums, the dilation reads the four neighbours of the flattened map through a
    zero-padded copy (the reference's linear offsets, the wrap into the next row included; the element past the map is no
    neighbour), the normalisation comes last.  Returns per level dict(u, v, idepth, color) in STEP5's scan order (idepth float64)."""
    L = len(ref_pyr)
    h0, w0 = ref_pyr[0].shape[:2]
    pix = u.astype(np.int64) + w0 * v.astype(np.int64)
    idm = [np.bincount(pix, weights=idp.astype(np.float64) * wgt.astype(np.float64), minlength=w0 * h0).reshape(h0, w0)]
    wsm = [np.bincount(pix, weights=wgt.astype(np.float64), minlength=w0 * h0).reshape(h0, w0)]
    for l in range(1, L):
        hl, wl = ref_pyr[l].shape[:2]
        idm.append(idm[-1][:2 * hl, :2 * wl].reshape(hl, 2, wl, 2).sum(axis=(1, 3)))
        wsm.append(wsm[-1][:2 * hl, :2 * wl].reshape(hl, 2, wl, 2).sum(axis=(1, 3)))
    out = []
    for l in range(L):
        hl, wl = idm[l].shape
        offs = (1 + wl, -1 - wl, wl - 1, -wl + 1) if l < 2 else (1, -1, wl, -wl)      # STEP3 diagonal, STEP4 axis neighbours
        idf, wsf = idm[l].reshape(-1).copy(), wsm[l].reshape(-1).copy()
        pad = wl + 1
        idpad, bak = np.pad(idf, pad), np.pad(wsf, pad)
        i = np.arange(wl, wl * hl - wl)
        s, num, cnt = np.zeros(len(i)), np.zeros(len(i)), np.zeros(len(i))
        for o in offs:
            j = pad + i + o
            nb = bak[j] > 0
            s += np.where(nb, idpad[j], 0.0)
            num += np.where(nb, bak[j], 0.0)
            cnt += nb
        fill = (wsf[i] <= 0) & (cnt > 0)
        idf[i[fill]] = s[fill] / cnt[fill]
        wsf[i[fill]] = num[fill] / cnt[fill]
        ys, xs = np.meshgrid(np.arange(2, hl - 2), np.arange(2, wl - 2), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        ws = wsf[xs + wl * ys]
        with np.errstate(divide="ignore", invalid="ignore"):
            idn = idf[xs + wl * ys] / ws
        col = ref_pyr[l][ys, xs, 0]
        keep = (ws > 0) & np.isfinite(col) & (idn > 0)
        out.append(dict(u=xs[keep], v=ys[keep], idepth=idn[keep], color=col[keep]))
    return out


def _random_pyramid(w, h, seed):
    rs = np.random.RandomState(seed)
    return synth.make_pyramid(rs.uniform(0, 255, (h, w)).astype(np.float32), synth.pyramid_levels(w, h))


def _assert_same_template(a, b):
    assert len(a) == len(b)
    for l in range(len(a)):
        for k in ("u", "v", "idepth", "color"):
            assert a[l][k].dtype == b[l][k].dtype == np.float32 and np.array_equal(a[l][k], b[l][k]), (l, k)


@pytest.mark.parametrize("shape", [(1232, 368), (640, 480)])
def test_make_coarse_depth_restatements_at_window_scale(oracle, shape):
    """orc_make_coarse_depth and synth.make_pc bit-identical at up to 20 000 points, with pixels shared across the 2048-point tiles,
    and on the edge inputs (border rows and columns, zero weights, zero and negative idepths)."""
    import pyoracle
    w, h = shape
    pyr = _random_pyramid(w, h, 11)
    for n, seed in ((1, 1), (257, 2), (2049, 3), (4097, 4), (20000, 5)):
        u, v, idp, wgt = helpers.splat_points(n, w, h, seed)
        a = synth.make_pc(u, v, idp, wgt, pyr)
        _assert_same_template(a, pyoracle.make_coarse_depth(oracle, u, v, idp, wgt, pyr))
        assert len(a[0]["u"]) > 0
    crossing = [g for g in helpers.pixel_groups(u, v, w) if g[0] // helpers.CD_TILE != g[-1] // helpers.CD_TILE]
    assert len(crossing) > 100 and max(len(g) for g in crossing) >= 32      # the n = 20 000 input: what the tiles have to get right
    u, v, idp, wgt = helpers.edge_points(3000, w, h, 6)
    a = synth.make_pc(u, v, idp, wgt, pyr)
    _assert_same_template(a, pyoracle.make_coarse_depth(oracle, u, v, idp, wgt, pyr))
    assert ((u == 0) | (v == h - 1)).any() and (wgt == 0).any() and (idp < 0).any()


@pytest.mark.parametrize("shape", [(1232, 368), (640, 480)])
def test_make_coarse_depth_against_f64_truth(shape):
    """The float restatement against coarse_depth_truth: the same pixels in the same order, the same colours, the normalised idepth
    within CD_BARS of the truth on every level."""
    w, h = shape
    pyr = _random_pyramid(w, h, 12)
    L = len(pyr)
    worst = np.zeros(L)
    for n, seed in ((257, 21), (2049, 22), (4097, 23), (20000, 24), (20000, 25)):
        u, v, idp, wgt = helpers.splat_points(n, w, h, seed)
        a = synth.make_pc(u, v, idp, wgt, pyr)
        t = coarse_depth_truth(u, v, idp, wgt, pyr)
        for l in range(L):
            assert len(t[l]["u"]) > 0
            assert np.array_equal(a[l]["u"], t[l]["u"].astype(np.float32)) and np.array_equal(a[l]["v"], t[l]["v"].astype(np.float32)), (n, l)
            assert np.array_equal(a[l]["color"], t[l]["color"]), (n, l)
            rel = np.abs(a[l]["idepth"].astype(np.float64) - t[l]["idepth"]) / t[l]["idepth"]
            worst[l] = max(worst[l], rel.max())
    assert (worst <= np.array(CD_BARS[:L])).all(), worst
    assert worst.max() > 0                              # the float path does round: the comparison is not vacuous

