"""GPU parity of the coarse tracker (BASELINE configs[0] and [1]) against the oracle, through the C-ABI.

Tolerances: inlier masks, point counts and n_warped are bit-exact; H, b, E differ only by the order
of the float sums (<= 2e-5 relative to the largest entry of the same kind, the reference itself
sums in float with carry buckets); pose after the full LM within 1e-5 (north_star)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prob_small():
    return synth.tracker_problem(w=640, h=480, npts=2000, seed=2001)        # configs[0]


@pytest.fixture(scope="module")
def prob_kitti():
    return synth.tracker_problem(w=1232, h=368, npts=2000, seed=2002)       # configs[1]


def _setup(ctx, prob, ref_slot, new_slot):
    ctx.upload_pyramid(new_slot, prob["pyr_new"])
    ctx.set_ref(ref_slot, prob["pc"])


def _cmp_eval(ctx, oracle, prob, prm, lvl, T, aff, repeat=1.0, ref_slot=1, new_slot=2):
    ev = abi.TrackEval()
    ctx.L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(*aff)), repeat, C.byref(ev))
    Ho, bo, reso, nwo, masko = helpers.oracle_eval(oracle, prob["pc"][lvl], prob["pyr_new"][lvl], ev)
    n = len(prob["pc"][lvl]["u"])
    H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0); mask = np.zeros(n, np.uint8)
    ctx.check(ctx.L.sdso_track_calc_res_gs(ctx.h, ref_slot, new_slot, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res), C.byref(nw), abi.bp(mask)))
    H = H.reshape(8, 8)
    assert np.array_equal(mask, masko)
    assert nw.value == nwo and res[1] == reso[1]
    assert res[5] == reso[5] or (np.isnan(res[5]) and np.isnan(reso[5]))   # 0/0 when nothing is in bounds, like the reference
    assert abs(res[0] - reso[0]) <= 2e-5 * abs(reso[0])
    assert np.allclose(res[2:5], reso[2:5], rtol=1e-4, atol=1e-7)
    assert np.abs(H - Ho).max() <= 2e-5 * np.abs(Ho).max()
    # entries of H and b span many decades after the SCALE_* scaling: compare per scale block too
    d = np.sqrt(np.abs(np.diag(Ho))) + 1e-30
    assert np.abs((H - Ho) / np.outer(d, d)).max() <= 5e-5
    assert np.abs((b - bo) / d).max() <= 5e-5 * max(1.0, np.abs(bo / d).max())
    return H, b, res, nw.value


def test_calc_res_gs_all_levels_640x480(gpu_ctx, oracle, prob_small):
    prob = prob_small
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    T = synth.se3_exp(np.array([0.015, -0.008, 0.3, 0.003, -0.005, 0.0015]))
    for lvl in range(prob["levels"]):
        _cmp_eval(gpu_ctx, oracle, prob, prm, lvl, T, (0.01, 1.0))
    # identity start (configs[0]: level 0, one GN iteration from identity)
    _cmp_eval(gpu_ctx, oracle, prob, prm, 0, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    # saturation path: tiny cutoff makes most residuals saturate
    _cmp_eval(gpu_ctx, oracle, prob, prm, 0, (np.eye(3), np.zeros(3)), (0.0, 0.0), repeat=0.05)


def test_calc_res_gs_kitti_all_levels(gpu_ctx, oracle, prob_kitti):
    prob = prob_kitti
    _setup(gpu_ctx, prob, 3, 4)
    prm = helpers.track_params(prob)
    rs = np.random.RandomState(9)
    for lvl in range(prob["levels"]):
        T = synth.se3_exp(np.array(prob_motion()) + rs.normal(0, 2e-3, 6))
        _cmp_eval(gpu_ctx, oracle, prob, prm, lvl, T, (0.02, 1.0), ref_slot=3, new_slot=4)


def prob_motion():
    return [0.02, -0.01, 0.35, 0.004, -0.006, 0.002]


def test_edge_cases(gpu_ctx, oracle, prob_small):
    prob = prob_small
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    # (a) every point out of bounds: huge translation -> zero inliers, zero H/b, n_warped 0
    T = (np.eye(3), np.array([500.0, 0.0, 0.0]))
    H, b, res, nw = _cmp_eval(gpu_ctx, oracle, prob, prm, 0, T, (0.0, 0.0))
    assert nw == 0 and not H.any()
    # (b) empty template level
    empty = dict(u=np.zeros(0, np.float32), v=np.zeros(0, np.float32), idepth=np.zeros(0, np.float32), color=np.zeros(0, np.float32))
    p2 = dict(prob)
    p2["pc"] = [empty] + list(prob["pc"][1:])
    gpu_ctx.set_ref(7, p2["pc"])
    _cmp_eval(gpu_ctx, oracle, p2, prm, 0, (np.eye(3), np.zeros(3)), (0.0, 0.0), ref_slot=7)
    # (c) ragged sizes: n = 1, 3, 65, 257 points (padding of n_warped to a multiple of 4)
    for n in (1, 3, 65, 257):
        sub = {k: v[:n] for k, v in prob["pc"][0].items()}
        p3 = dict(prob)
        p3["pc"] = [sub] + list(prob["pc"][1:])
        gpu_ctx.set_ref(8, p3["pc"])
        _cmp_eval(gpu_ctx, oracle, p3, prm, 0, (np.eye(3), np.zeros(3)), (0.0, 0.0), ref_slot=8)
    # (d) error behaviour: unknown slots and a w/h mismatch are refused, not executed
    ev = abi.TrackEval()
    gpu_ctx.L.sdso_track_make_eval(C.byref(prm), 0, C.byref(abi.SE3.from_Rt(np.eye(3), np.zeros(3))), C.byref(abi.Aff(0, 0)), 1.0, C.byref(ev))
    assert gpu_ctx.L.sdso_track_calc_res_gs(gpu_ctx.h, 999, 2, C.byref(ev), None, None, None, None, None) == -1
    ev.w += 2
    assert gpu_ctx.L.sdso_track_calc_res_gs(gpu_ctx.h, 1, 2, C.byref(ev), None, None, None, None, None) == -1


def test_batch_matches_single(gpu_ctx, oracle, prob_small, prob_kitti):
    _setup(gpu_ctx, prob_small, 1, 2)
    _setup(gpu_ctx, prob_kitti, 3, 4)
    rs = np.random.RandomState(4)
    evs, refs, frames, exp = [], [], [], []
    for i in range(19):   # not a multiple of 8: exercises the XCD-group tail
        prob, r, f = (prob_small, 1, 2) if i % 2 == 0 else (prob_kitti, 3, 4)
        prm = helpers.track_params(prob)
        lvl = i % prob["levels"]
        T = synth.se3_exp(np.array(prob_motion()) + rs.normal(0, 3e-3, 6))
        ev = abi.TrackEval()
        gpu_ctx.L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(0.01, 0.5)), 1.0, C.byref(ev))
        evs.append(ev); refs.append(r); frames.append(f)
        exp.append(helpers.oracle_eval(oracle, prob["pc"][lvl], prob["pyr_new"][lvl], ev))
    n = len(evs)
    arr = (abi.TrackEval * n)(*evs)
    H = np.zeros((n, 64)); b = np.zeros((n, 8)); res = np.zeros((n, 6)); nw = np.zeros(n, np.int32)
    gpu_ctx.check(gpu_ctx.L.sdso_track_calc_res_gs_batch(gpu_ctx.h, n, abi.ip(np.array(refs, np.int32)), abi.ip(np.array(frames, np.int32)),
                                                         arr, abi.dp(H), abi.dp(b), abi.dp(res), abi.ip(nw)))
    for i in range(n):
        Ho, bo, reso, nwo, _ = exp[i]
        assert nw[i] == nwo and res[i, 1] == reso[1]
        assert np.abs(H[i].reshape(8, 8) - Ho).max() <= 2e-5 * np.abs(Ho).max()
        assert abs(res[i, 0] - reso[0]) <= 2e-5 * abs(reso[0])


@pytest.mark.parametrize("which", ["small", "kitti"])
def test_track_newest_coarse_pose_within_1e5(gpu_ctx, oracle, prob_small, prob_kitti, which):
    prob = prob_small if which == "small" else prob_kitti
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    To, affo, outo = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, 1, 2, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    assert out.good == outo.good == 1
    assert list(out.iterations) == list(outo.iterations) and out.evaluations == outo.evaluations and out.point_evals == outo.point_evals
    R, t = T.Rt(); Ro, to = To.Rt()
    assert np.abs(t - to).max() <= 1e-5 and np.abs(R - Ro).max() <= 1e-5          # north_star: pose deltas within 1e-5
    assert abs(aff.a - affo.a) <= 1e-5 and abs(aff.b - affo.b) <= 1e-3
    for l in range(prob["levels"]):
        assert abs(out.lastResiduals[l] - outo.lastResiduals[l]) <= 1e-4 * outo.lastResiduals[l]
    Rt, tt = prob["refToNew_true"]
    assert np.abs(t - tt).max() < 5e-3                                          # and it is the right pose


def test_track_abort_and_error(gpu_ctx, oracle, prob_small):
    prob = prob_small
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    for i in range(5):
        prm.minResForAbort[i] = 0.01
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, 1, 2, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    To, affo, outo = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    assert out.good == outo.good == 0 and np.array_equal(T.Rt()[0], np.eye(3))
    assert np.isnan(out.lastResiduals[0])
    prm.coarsestLvl = 7
    assert gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, 1, 2, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)) == -1


def test_tracker_refusals(gpu_ctx, prob_small):
    """The four entry points that evaluate a template level on an image level — sdso_track_calc_res_gs, sdso_track_newest_coarse,
    sdso_g2o_track_add_edges, sdso_g2o_track_linearize — refuse an unknown reference slot, an unknown frame slot, a level outside the
    uploaded pyramid and a w or h one off the uploaded level's with SDSO_ERR_ARG, before anything is launched; the same correct calls
    before and after the refusals give the same bits (every reduction on these paths runs in a fixed order)."""
    from test_g2o_factors import _g2o_eval
    prob, L, h = prob_small, gpu_ctx.L, gpu_ctx.h
    ERR_ARG = -1
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    top = prm.coarsestLvl                                          # the level a trackNewestCoarse call starts on
    assert top == prob["levels"] - 1 >= 3
    gpu_ctx.upload_pyramid(5, prob["pyr_new"][:top])               # the same image without its coarsest level
    T0 = synth.se3_exp(np.array([0.015, -0.008, 0.3, 0.003, -0.005, 0.0015]))
    lvl = 1
    n = len(prob["pc"][lvl]["u"])

    def make_ev(**over):
        ev = abi.TrackEval()
        L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T0)), C.byref(abi.Aff(0.01, 1.0)), 1.0, C.byref(ev))
        for k, v in over.items():
            setattr(ev, k, v)
        return ev

    def make_evg(**over):
        ev = _g2o_eval(L, "sdso_", prm, lvl, T0, T0, (0.01, 1.0))
        for k, v in over.items():
            setattr(ev, k, v)
        return ev

    def calc(ref, frame, ev):
        H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0); mask = np.zeros(n, np.uint8)
        rc = L.sdso_track_calc_res_gs(h, ref, frame, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res), C.byref(nw), abi.bp(mask))
        return rc, (H, b, res, nw.value, mask)

    def track(ref, frame, p):
        T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
        rc = L.sdso_track_newest_coarse(h, ref, frame, C.byref(p), C.byref(T), C.byref(aff), C.byref(out))
        return rc, (bytes(T), bytes(aff), out.good, list(out.iterations), out.evaluations, out.point_evals,
                    np.array(out.lastResiduals), np.array(out.lastFlowIndicators))

    def add_edges(ref, frame, ev):
        res = np.zeros(6); ne = C.c_int(0); mask = np.zeros(n, np.uint8); X = np.zeros((n, 3), np.float32)
        rc = L.sdso_g2o_track_add_edges(h, ref, frame, C.byref(ev), abi.dp(res), C.byref(ne), abi.bp(mask), abi.fp(X))
        return rc, (res, ne.value, mask, X)

    def linearize(ref, frame, ev):
        H = np.zeros(64); b = np.zeros(8); chi = np.zeros(2)
        rc = L.sdso_g2o_track_linearize(h, ref, frame, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(chi), None, None)
        return rc, (H, b, chi)

    def good_calls():
        got = []
        for rc, val in (calc(1, 2, make_ev()), track(1, 2, prm), add_edges(1, 2, make_evg()), linearize(1, 2, make_evg())):
            assert rc == 0
            got.append(val)
        return got

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) else a == b

    before = good_calls()
    assert before[0][3] > 0 and before[2][1] > 0                    # the correct calls evaluate something

    w1, h1 = prob["pyr_new"][lvl].shape[1], prob["pyr_new"][lvl].shape[0]
    # (reference slot, frame slot, overrides of the evaluation's lvl / w / h)
    ev_cases = [(999, 2, {}), (1, 998, {}), (1, 2, dict(lvl=prob["levels"])), (1, 2, dict(lvl=-1)), (1, 5, dict(lvl=top)),
                (1, 2, dict(w=w1 + 1)), (1, 2, dict(w=w1 - 1)), (1, 2, dict(h=h1 + 1)), (1, 2, dict(h=h1 - 1))]
    for ref, frame, over in ev_cases:
        assert calc(ref, frame, make_ev(**over))[0] == ERR_ARG, ("calc_res_gs", ref, frame, over)
        assert add_edges(ref, frame, make_evg(**over))[0] == ERR_ARG, ("add_edges", ref, frame, over)
        assert linearize(ref, frame, make_evg(**over))[0] == ERR_ARG, ("linearize", ref, frame, over)   # (999: no edge set of that reference)

    def params(level=None, dw=0, dh=0):
        p = helpers.track_params(prob)
        if level is not None:
            p.w[level] += dw; p.h[level] += dh
        return p
    trk_cases = [(999, 2, params()), (1, 998, params()), (1, 5, params()),      # (slot 5 lacks the level the call starts on)
                 (1, 2, params(0, dw=1)), (1, 2, params(2, dw=-1)), (1, 2, params(top, dh=1)), (1, 2, params(1, dh=-1))]
    for k, (ref, frame, p) in enumerate(trk_cases):
        assert track(ref, frame, p)[0] == ERR_ARG, ("newest_coarse", k)

    assert same(before, good_calls())


def test_make_pyramid_bit_exact(gpu_ctx, oracle, prob_kitti):
    img = np.ascontiguousarray(prob_kitti["pyr_new"][0][..., 0])
    h, w = img.shape
    gpu_ctx.check(gpu_ctx.L.sdso_make_pyramid(gpu_ctx.h, 11, w, h, abi.fp(img)))
    for l in range(prob_kitti["levels"]):
        out = np.zeros((h >> l, w >> l, 3), np.float32)
        gpu_ctx.check(gpu_ctx.L.sdso_download_pyramid_level(gpu_ctx.h, 11, l, abi.fp(out)))
        assert np.array_equal(out, prob_kitti["pyr_new"][l])
    # upload -> download round trip
    gpu_ctx.upload_pyramid(12, prob_kitti["pyr_ref"])
    out = np.zeros_like(prob_kitti["pyr_ref"][2])
    gpu_ctx.check(gpu_ctx.L.sdso_download_pyramid_level(gpu_ctx.h, 12, 2, abi.fp(out)))
    assert np.array_equal(out, prob_kitti["pyr_ref"][2])


def test_make_ref_bit_exact_bookkeeping(gpu_ctx, oracle):
    """CoarseTracker::makeCoarseDepthL0 STEP1-5 on the device (sdso_track_make_ref) against the oracle's C++ restatement
    (oracle/orc_tracker.cpp::orc_make_coarse_depth, CoarseTracker.cpp:352-534): pc_n of every level, the ORDER of the template points and every float
    must be identical — this is the tracker's point-index bookkeeping.  The input has pixels hit by 2, 3 and 5 points
    with different weights (the splat must add them in point order).  Its 1500 points fill one 2048-point tile of k_cd_splat, so
    collisions across tiles are left to tests/test_tracking_ref_gpu.py."""
    prob = synth.tracker_problem(w=640, h=480, npts=1500, seed=2031)
    u, v, idp = prob["points"]
    rs = np.random.RandomState(3)
    u = u.astype(np.int32).copy(); v = v.astype(np.int32).copy(); idp = idp.astype(np.float32).copy()
    for dst, src in ((10, 500), (11, 500), (12, 500), (13, 500), (20, 700), (21, 700), (30, 900), (1400, 3), (1401, 3)):
        u[dst], v[dst] = u[src], v[src]                       # collisions, also across 256-thread workgroups
    wgt = rs.uniform(0.2, 3.0, len(u)).astype(np.float32)
    idp = (idp * rs.uniform(0.9, 1.1, len(u))).astype(np.float32)
    import pyoracle
    exp = pyoracle.make_coarse_depth(oracle, u, v, idp, wgt, prob["pyr_ref"])
    gpu_ctx.upload_pyramid(21, prob["pyr_ref"])
    L = prob["levels"]
    pcn = np.zeros(8, np.int32)
    gpu_ctx.check(gpu_ctx.L.sdso_track_make_ref(gpu_ctx.h, 31, 21, len(u), abi.ip(u), abi.ip(v), abi.fp(idp), abi.fp(wgt), abi.ip(pcn)))
    for l in range(L):
        n = len(exp[l]["u"])
        assert pcn[l] == n and n > 0
        got = [np.zeros(n, np.float32) for _ in range(4)]
        nn = C.c_int(0)
        gpu_ctx.check(gpu_ctx.L.sdso_track_get_ref(gpu_ctx.h, 31, l, C.byref(nn), *[abi.fp(a) for a in got]))
        assert nn.value == n
        for a, k in zip(got, ("u", "v", "idepth", "color")):
            assert np.array_equal(a, exp[l][k]), (l, k)
    # the installed reference tracks like one set with sdso_track_set_ref
    gpu_ctx.upload_pyramid(22, prob["pyr_new"])
    p2 = dict(prob); p2["pc"] = exp
    gpu_ctx.set_ref(32, exp)
    prm = helpers.track_params(p2)
    res = []
    for ref in (31, 32):
        T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
        gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, ref, 22, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
        res.append((T.Rt(), aff.a, aff.b, out.good))
    assert np.array_equal(res[0][0][0], res[1][0][0]) and np.array_equal(res[0][0][1], res[1][0][1]) and res[0][1:] == res[1][1:]
    # empty input: every level empty, nothing faults
    gpu_ctx.check(gpu_ctx.L.sdso_track_make_ref(gpu_ctx.h, 33, 21, 0, None, None, None, None, abi.ip(pcn)))
    assert (pcn[:L] == 0).all()


def test_track_hypotheses_in_lock_step(gpu_ctx, oracle, prob_small, prob_kitti):
    """sdso_track_newest_coarse_batch: the motion hypotheses FullSystem::trackNewCoarse tries one after the other
    (FullSystem.cpp:305-441), all advanced together.  Each hypothesis must end where the sequential oracle ends."""
    _setup(gpu_ctx, prob_small, 1, 2)
    _setup(gpu_ctx, prob_kitti, 3, 4)
    rs = np.random.RandomState(17)
    hyps = []
    for k in range(9):
        prob, r, f = (prob_small, 1, 2) if k % 3 else (prob_kitti, 3, 4)
        xi = np.zeros(6) if k < 2 else rs.normal(0, [0.02, 0.02, 0.1, 0.003, 0.003, 0.003])
        if k == 8:
            xi = np.array([3.0, 0, 0, 0, 0.5, 0])            # a hopeless start: must come back not good without disturbing the others
        hyps.append((prob, r, f, synth.se3_exp(xi)))
    n = len(hyps)
    prms = (abi.TrackParams * n)(*[helpers.track_params(h[0]) for h in hyps])
    for k in range(n):
        for i in range(5):
            prms[k].minResForAbort[i] = 1e3 if k != 4 else 0.01   # hypothesis 4 aborts on its first level
    Ts = (abi.SE3 * n)(*[abi.SE3.from_Rt(*h[3]) for h in hyps])
    affs = (abi.Aff * n)(*[abi.Aff(0, 0) for _ in hyps])
    outs = (abi.TrackResult * n)()
    refs = np.array([h[1] for h in hyps], np.int32); frames = np.array([h[2] for h in hyps], np.int32)
    gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse_batch(gpu_ctx.h, n, abi.ip(refs), abi.ip(frames), prms, Ts, affs, outs))
    ngood = 0
    for k, (prob, r, f, T0) in enumerate(hyps):
        To, affo, outo = helpers.oracle_track(oracle, prob, prms[k], T0, (0.0, 0.0))
        assert outs[k].good == outo.good, k
        if k == 8:          # almost no inliers: the 8x8 system is near-singular and amplifies the order of the float sums; only the verdict is compared
            continue
        assert list(outs[k].iterations) == list(outo.iterations) and outs[k].evaluations == outo.evaluations, k
        R, t = Ts[k].Rt(); Ro, to = To.Rt()
        assert np.abs(t - to).max() <= 1e-5 and np.abs(R - Ro).max() <= 1e-5, k
        assert abs(affs[k].a - affo.a) <= 1e-5 and abs(affs[k].b - affo.b) <= 1e-3, k
        ngood += outs[k].good
    assert outs[4].good == 0 and np.array_equal(Ts[4].Rt()[0], hyps[4][3][0])      # aborted: pose untouched
    assert ngood >= 6


def test_cluster_sizes_reproduce_the_iteration_counts(gpu_ctx, oracle, prob_small, prob_kitti, monkeypatch):
    """k_track_lm spreads a hypothesis over a cluster of G workgroups; G follows the device's occupancy, and the split of the points
    changes the order of the float sums.  The LM iteration / evaluation counts are bookkeeping the caller sees: for EVERY cluster size
    1..8, on eight hypotheses in one call, they must be the oracle's — except where the oracle itself sat on a decision threshold: a level
    whose counts differ must have taken an accept / stop / repeat decision with a relative margin below 1e-5 (the size of the order-of-
    summation differences in E / n; measured margins of the decisions that do NOT flip: > 1e-4).  Poses agree to 1e-5 either way."""
    _setup(gpu_ctx, prob_small, 1, 2)
    _setup(gpu_ctx, prob_kitti, 3, 4)
    rs = np.random.RandomState(29)
    hyps = []
    for k in range(8):
        prob, r, f = (prob_small, 1, 2) if k % 2 else (prob_kitti, 3, 4)
        xi = np.zeros(6) if k < 2 else rs.normal(0, [0.02, 0.02, 0.1, 0.003, 0.003, 0.003])
        hyps.append((prob, r, f, synth.se3_exp(xi)))
    n = len(hyps)
    prms = (abi.TrackParams * n)(*[helpers.track_params(h[0]) for h in hyps])
    ref = []
    for k, (prob, r, f, T0) in enumerate(hyps):
        To, affo, outo = helpers.oracle_track(oracle, prob, prms[k], T0, (0.0, 0.0))
        m = np.zeros(5)
        oracle.orc_track_last_margins(abi.dp(m))
        ref.append((To, affo, outo, m))
    refs = np.array([h[1] for h in hyps], np.int32); frames = np.array([h[2] for h in hyps], np.int32)
    flips = 0
    for G in range(1, 9):
        monkeypatch.setenv("SDSO_TRK_LM_CLUSTER", str(G))
        Ts = (abi.SE3 * n)(*[abi.SE3.from_Rt(*h[3]) for h in hyps])
        affs = (abi.Aff * n)(*[abi.Aff(0, 0) for _ in hyps])
        outs = (abi.TrackResult * n)()
        gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse_batch(gpu_ctx.h, n, abi.ip(refs), abi.ip(frames), prms, Ts, affs, outs))
        for k in range(n):
            To, affo, outo, m = ref[k]
            assert outs[k].good == outo.good, (G, k)
            R, t = Ts[k].Rt(); Ro, to = To.Rt()
            assert np.abs(t - to).max() <= 1e-5 and np.abs(R - Ro).max() <= 1e-5, (G, k)
            if list(outs[k].iterations) != list(outo.iterations) or outs[k].evaluations != outo.evaluations:
                flips += 1
                lv = [l for l in range(5) if outs[k].iterations[l] != outo.iterations[l]]
                # counts can only diverge from the first level on which the oracle took a knife-edge decision
                assert lv and min(m[l] for l in range(max(lv), 5)) <= 1e-5, (G, k, list(outs[k].iterations), list(outo.iterations), m)
    monkeypatch.delenv("SDSO_TRK_LM_CLUSTER")
    assert flips <= 2                                   # (none on these problems at the time of writing)


@pytest.mark.parametrize("modes", [(-1.0, -1.0), (0.0, 0.0), (-1.0, 1e8), (1e12, -1.0)])
def test_track_affine_modes(gpu_ctx, oracle, prob_small, modes):
    """setting_affineOptModeA/B variants (main_dso_pangolin.cpp:315-338: mode 1 sets both 0, mode 2 sets both -1): the LM solves the
    reduced 6 / 7-parameter systems (CoarseTracker.cpp:937-964) and the final affine sanity checks differ (:1050-1066)."""
    prob = prob_small
    _setup(gpu_ctx, prob, 1, 2)
    prm = helpers.track_params(prob)
    prm.affineOptModeA, prm.affineOptModeB = modes
    To, affo, outo = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, 1, 2, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    assert out.good == outo.good
    assert list(out.iterations) == list(outo.iterations) and out.evaluations == outo.evaluations
    R, t = T.Rt(); Ro, to = To.Rt()
    assert np.abs(t - to).max() <= 1e-5 and np.abs(R - Ro).max() <= 1e-5
    assert abs(aff.a - affo.a) <= 1e-5 and abs(aff.b - affo.b) <= 1e-3
    if modes[0] < 0:
        assert aff.a == 0.0
    if modes[1] < 0:
        assert aff.b == 0.0


def test_full_size_linearity(gpu_ctx, prob_kitti):
    """configs[1] size, a size-independent property: calcRes+calcGSSSE is a sum over template points, so the un-normalised Hessian
    n*H, n*b and the energy of a template equal the sums over its two halves (even / odd points), and the inlier counts add."""
    prob = prob_kitti
    gpu_ctx.upload_pyramid(4, prob["pyr_new"])
    prm = helpers.track_params(prob)
    T = synth.se3_exp(np.array(prob_motion()))
    for lvl in (0, 2):
        pc = prob["pc"][lvl]
        halves = [{k: v[i::2] for k, v in pc.items()} for i in range(2)]
        res = []
        for slot, sub in ((70, pc), (71, halves[0]), (72, halves[1])):
            pcs = [dict(u=np.zeros(0, np.float32), v=np.zeros(0, np.float32), idepth=np.zeros(0, np.float32), color=np.zeros(0, np.float32))] * prob["levels"]
            pcs = list(pcs); pcs[lvl] = sub
            gpu_ctx.set_ref(slot, pcs)
            ev = abi.TrackEval()
            gpu_ctx.L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(0.02, 1.0)), 1.0, C.byref(ev))
            H = np.zeros(64); b = np.zeros(8); r = np.zeros(6); nw = C.c_int(0); mask = np.zeros(len(sub["u"]), np.uint8)
            gpu_ctx.check(gpu_ctx.L.sdso_track_calc_res_gs(gpu_ctx.h, slot, 4, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(r), C.byref(nw), abi.bp(mask)))
            n_in = int(mask.sum())
            res.append((H * n_in, b * n_in, r[0], r[1], n_in, mask))
        (Hf, bf, Ef, nf_, cf, mf), (Ha, ba, Ea, na, ca, ma), (Hb, bb, Eb, nb, cb, mb) = res
        assert cf == ca + cb and nf_ == na + nb
        assert np.array_equal(mf[0::2], ma) and np.array_equal(mf[1::2], mb)                 # the same points are inliers
        assert abs(Ef - (Ea + Eb)) <= 2e-5 * Ef
        assert np.abs(Hf - (Ha + Hb)).max() <= 5e-5 * np.abs(Hf).max()
        d = np.sqrt(np.abs(np.diag(Hf.reshape(8, 8)))) + 1e-30
        assert np.abs((bf - (ba + bb)) / d).max() <= 5e-5 * max(1.0, np.abs(bf / d).max())
