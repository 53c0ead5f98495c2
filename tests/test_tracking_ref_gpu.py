"""The keyframe's tracking template built on the device, and the stereo batches that feed it, at window scale.

* sdso_track_make_ref (CoarseTracker::makeCoarseDepthL0 STEP1-splat .. STEP5, csrc/coarse_depth.hip).  k_cd_splat adds the points
  that share a pixel in point order, reading earlier points through LDS tiles of 2048: a point looks for an earlier owner of its
  pixel in every earlier tile, and the owner adds the later points of its pixel from every later tile.  Both loops only cross a
  tile beyond 2048 points; the window aims at 4000 (setting_desiredPointDensity, settings.cpp:60).  pc_n, the order of the points
  and every float must equal both float restatements, orc_make_coarse_depth and synth.make_pc, at 1232x368 and 640x480.  Those two
  are pinned to each other and to a float64 truth in tests/test_oracle_tracker.py, which records the truth's bars.
* sdso_stereo_match_batch (the L->R->L chain of makeCoarseDepthL0 STEP1 and FullSystem::stereoMatch) at the bench's match shape,
  both search directions, against the oracle's four steps; then STEP1 end to end: match, accept rule, weight, template.
* The benchmarked traceStereo path (sdso_trace_stereo_prepare / _enqueue / _fetch).  Every enqueue restores idepth_min_stereo,
  idepth_max_stereo, quality and lastTraceStatus from the copies prepare made, so repeated enqueues trace the same input.

The module has its own context: it switches the trace refinement mode and grows the stereo batches."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth
from test_stereo import FIELDS, _oracle_init, _oracle_trace

pytestmark = pytest.mark.gpu

SHAPES = ((1232, 368), (640, 480))
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, 20000)
KEYS = ("u", "v", "idepth", "color")
REF_FRAME = {(1232, 368): 1, (640, 480): 2}      # frame slots of the template pyramids
NEW_FRAME = 3                                     # the 1232x368 frame that is tracked against a template
LEFT, RIGHT = 80, 81                              # the bench's stereo pair


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    out = {}
    for (w, h) in SHAPES:
        out[(w, h)] = synth.tracker_problem(w=w, h=h, npts=4000, seed=2201)
        ctx.upload_pyramid(REF_FRAME[(w, h)], out[(w, h)]["pyr_ref"])
    ctx.upload_pyramid(NEW_FRAME, out[(1232, 368)]["pyr_new"])
    return out


def make_ref(ctx, slot, frame, u, v, idp, wgt):
    u, v = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32)
    idp, wgt = np.ascontiguousarray(idp, np.float32), np.ascontiguousarray(wgt, np.float32)
    pcn = np.zeros(8, np.int32)
    ctx.check(ctx.L.sdso_track_make_ref(ctx.h, slot, frame, len(u), abi.ip(u), abi.ip(v), abi.fp(idp), abi.fp(wgt), abi.ip(pcn)))
    return pcn


def get_ref(ctx, slot, levels):
    out = []
    for l in range(levels):
        nn = C.c_int(-1)
        ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), None, None, None, None))
        arrs = [np.zeros(nn.value, np.float32) for _ in KEYS]
        if nn.value:
            ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), *[abi.fp(a) for a in arrs]))
        out.append(dict(zip(KEYS, arrs)))
    return out


def check_make_ref(ctx, oracle, slot, frame, pyr, u, v, idp, wgt):
    """make_ref on the device == orc_make_coarse_depth == synth.make_pc: pc_n, order, every float of every level"""
    import pyoracle
    exp_o = pyoracle.make_coarse_depth(oracle, u, v, idp, wgt, pyr)
    exp_s = synth.make_pc(u, v, idp, wgt, pyr)
    pcn = make_ref(ctx, slot, frame, u, v, idp, wgt)
    got = get_ref(ctx, slot, len(pyr))
    for l in range(len(pyr)):
        assert pcn[l] == len(got[l]["u"]) == len(exp_o[l]["u"]) == len(exp_s[l]["u"]), (l, pcn[l], len(exp_o[l]["u"]))
        for k in KEYS:
            assert np.array_equal(got[l][k], exp_o[l][k]), (l, k)
            assert np.array_equal(got[l][k], exp_s[l][k]), (l, k)
    return exp_o


def crossing_groups(u, v, w):
    return [g for g in helpers.pixel_groups(u, v, w) if g[0] // helpers.CD_TILE != g[-1] // helpers.CD_TILE]


# ------------------------------------------------------------------ sdso_track_make_ref
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=["1232x368", "640x480"])
def test_make_ref_sizes(ctx, oracle, scenes, shape, n):
    """Around the 256-point workgroup and the 2048-point tile, and at 20 000 points: pairs across every workgroup edge, first hits in
    one tile with later hits in later tiles (the last point among them), 40 points on one pixel spread over every tile."""
    w, h = shape
    u, v, idp, wgt = helpers.splat_points(n, w, h, seed=n)
    if n > helpers.CD_TILE:
        assert crossing_groups(u, v, w)
    if n == 20000:
        g = max(helpers.pixel_groups(u, v, w), key=len)
        assert len(g) >= 32 and len(set(g // helpers.CD_TILE)) == -(-n // helpers.CD_TILE)
    check_make_ref(ctx, oracle, 10, REF_FRAME[shape], scenes[shape]["pyr_ref"], u, v, idp, wgt)


@pytest.mark.parametrize("shape", SHAPES, ids=["1232x368", "640x480"])
def test_make_ref_natural_collisions(ctx, oracle, scenes, shape):
    """The points of a keyframe window projected into its newest keyframe, rounded and splatted frame by frame as STEP1 does: the
    collisions come from the geometry, some of them across tiles."""
    w, h = shape
    win = synth.ba_window(w=w, h=h, nf=6, pts_per_kf=700, seed=3301)
    u, v, idp, wgt, _ = helpers.window_points(win, seed=5)
    assert 3000 < len(u) < 4200 and (idp > 0).all()
    assert len(helpers.pixel_groups(u, v, w)) >= 20 and crossing_groups(u, v, w)
    ctx.upload_pyramid(20, win["pyrs"][-1])
    check_make_ref(ctx, oracle, 11, 20, win["pyrs"][-1], u, v, idp, wgt)


@pytest.mark.parametrize("shape", SHAPES, ids=["1232x368", "640x480"])
def test_make_ref_edge_inputs(ctx, oracle, scenes, shape):
    """Points on the border rows and columns, zero weights, zero and negative idepths, and a reference image with non-finite colours
    under kept pixels of every level (STEP5 drops them)."""
    w, h = shape
    u, v, idp, wgt = helpers.edge_points(5000, w, h, seed=41)
    shared = helpers.pixel_groups(u, v, w)
    assert any((wgt[g] == 0).any() and (wgt[g] > 0).any() for g in shared) and any((idp[g] < 0).any() and (idp[g] > 0).any() for g in shared)
    pyr = [p.copy() for p in scenes[shape]["pyr_ref"]]
    for l, p in enumerate(pyr):
        hl, wl = p.shape[:2]
        p[(v[:300] >> l).clip(2, hl - 3), (u[:300] >> l).clip(2, wl - 3), 0] = np.nan
    ctx.upload_pyramid(21, pyr)
    check_make_ref(ctx, oracle, 12, 21, pyr, u, v, idp, wgt)


def test_make_ref_slot_lifecycle(ctx, oracle, scenes):
    """The same slot rebuilt: a large template, then a small one; a template made over one installed by sdso_track_set_ref, and a
    4-level template over a 5-level one (the fifth level must be gone)."""
    big, small = (1232, 368), (640, 480)
    pyr = scenes[big]["pyr_ref"]
    check_make_ref(ctx, oracle, 13, REF_FRAME[big], pyr, *helpers.splat_points(20000, *big, seed=51))
    check_make_ref(ctx, oracle, 13, REF_FRAME[big], pyr, *helpers.splat_points(257, *big, seed=52))
    ctx.set_ref(14, scenes[big]["pc"])
    check_make_ref(ctx, oracle, 14, REF_FRAME[big], pyr, *helpers.splat_points(4097, *big, seed=53))
    ctx.set_ref(15, scenes[big]["pc"])
    assert len(get_ref(ctx, 15, 5)[4]["u"]) > 0
    check_make_ref(ctx, oracle, 15, REF_FRAME[small], scenes[small]["pyr_ref"], *helpers.splat_points(4097, *small, seed=54))
    assert len(get_ref(ctx, 15, 5)[4]["u"]) == 0


def test_made_ref_tracks_like_set_ref(ctx, oracle, scenes):
    """sdso_track_newest_coarse on the template make_ref built == on the expected template installed with set_ref, bit for bit, at
    1232x368 (window-sized input: the scene's 4000 points with noisy idepths and weights, a few dozen of them on shared pixels)."""
    prob = scenes[(1232, 368)]
    u, v, idp = [np.array(a) for a in prob["points"]]
    u, v = u.astype(np.int32), v.astype(np.int32)
    rs = np.random.RandomState(61)
    idp = (idp * rs.uniform(0.95, 1.05, len(u))).astype(np.float32)
    wgt = np.sqrt((1e-3 / (rs.uniform(2e-4, 2e-2, len(u)) + 1e-12)).astype(np.float32)).astype(np.float32)
    for dst in range(2100, 2140):
        u[dst], v[dst] = u[dst - 2048], v[dst - 2048]
    exp = check_make_ref(ctx, oracle, 16, REF_FRAME[(1232, 368)], prob["pyr_ref"], u, v, idp, wgt)
    ctx.set_ref(17, exp)
    p2 = dict(prob)
    p2["pc"] = exp
    prm = helpers.track_params(p2)
    res = []
    for ref in (16, 17):
        T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
        ctx.check(ctx.L.sdso_track_newest_coarse(ctx.h, ref, NEW_FRAME, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
        res.append((T.Rt(), aff.a, aff.b, out.good, out.evaluations, list(out.lastResiduals)))
    (R0, t0), (R1, t1) = res[0][0], res[1][0]
    assert np.array_equal(R0, R1) and np.array_equal(t0, t1) and res[0][1:] == res[1][1:]
    assert res[0][3] == 1 and np.abs(t0 - prob["refToNew_true"][1]).max() < 5e-3


# ------------------------------------------------------------------ sdso_stereo_match_batch at the bench shape
@pytest.fixture(scope="module")
def kitti(ctx):
    """bench.py MatchWorkload / TraceWorkload: 1232x368, 20 000 points, seed 4001; plus 20 000 points of the right image and their
    inverse depths there, for matches that start on the right."""
    pr = synth.stereo_problem(w=1232, h=368, npts=20000, seed=4001)
    ur, vr = synth.select_points(pr["pyr_r"][0], 20000, 4001, margin=6)
    _, id_r = synth.Scene(1001).render(pr["w"], pr["h"], pr["K"], (np.eye(3), np.array([-float(pr["calib"]["baseline"]), 0.0, 0.0])))
    pr["ur"], pr["vr"], pr["idepth_true_r"] = ur.astype(np.float32), vr.astype(np.float32), id_r[vr, ur].astype(np.float32)
    pr["K32"], pr["bl"] = np.array(pr["K"], np.float32), float(pr["calib"]["baseline"])
    ctx.upload_pyramid(LEFT, pr["pyr_l"]); ctx.upload_pyramid(RIGHT, pr["pyr_r"])
    return pr


def oracle_match(oracle, pr, mode_first, u, v, imin, imax):
    """the oracle's four steps: ctor on frame A, trace in frame B, ctor at lastTraceUV on frame B, trace back in frame A"""
    img_l, img_r = np.ascontiguousarray(pr["pyr_l"][0]), np.ascontiguousarray(pr["pyr_r"][0])
    img_a, img_b = (img_l, img_r) if mode_first else (img_r, img_l)
    co, wo, go, eo = _oracle_init(oracle, pr, img_a, u, v)
    Pf, df = abi.make_trace_points(len(u), u, v, co, wo, go, eo, imin, imax)
    sf = _oracle_trace(oracle, pr, img_b, Pf, mode_first)
    good = np.nonzero(sf == 0)[0]
    ub, vb = df["lastTraceUV"][good, 0].copy(), df["lastTraceUV"][good, 1].copy()
    c2, w2, g2, e2 = _oracle_init(oracle, pr, img_b, ub, vb)
    Pb, db = abi.make_trace_points(len(good), ub, vb, c2, w2, g2, e2, None if imin is None else imin[good], None if imax is None else imax[good])
    sb = _oracle_trace(oracle, pr, img_a, Pb, 1 - mode_first)
    return sf, df, good, sb, db


def device_match(c, pr, mode_first, u, v, imin, imax):
    n = len(u)
    out = dict(status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), idepth_stereo=np.zeros(n, np.float32),
               idepth_min_out=np.zeros(n, np.float32), idepth_max_out=np.zeros(n, np.float32), fwd_uv=np.zeros((n, 2), np.float32),
               back_uv=np.zeros((n, 2), np.float32))
    M = abi.StereoMatch()
    M.n = n; M.u = abi.fp(u); M.v = abi.fp(v)
    if imin is not None:
        M.idepth_min_stereo = abi.fp(imin); M.idepth_max_stereo = abi.fp(imax)
        M.back_idepth_min_stereo = abi.fp(imin); M.back_idepth_max_stereo = abi.fp(imax)
    abi.bind(M, out)
    slots = (LEFT, RIGHT) if mode_first else (RIGHT, LEFT)
    c.check(c.L.sdso_stereo_match_batch(c.h, slots[0], slots[1], abi.fp(pr["K32"]), pr["bl"], mode_first, C.byref(M)))
    return out


def match_case(pr, mode_first, interval, idx=None):
    """points of frame A (left for mode_right_first = 1, right for 0), optionally with the prior interval 0.1 .. 1.9 x the true
    inverse depth (makeCoarseDepthL0 STEP1, CoarseTracker.cpp:312-313)"""
    u, v, idt = (pr["u"], pr["v"], pr["idepth_true"]) if mode_first else (pr["ur"], pr["vr"], pr["idepth_true_r"])
    idx = np.arange(len(u)) if idx is None else idx
    u, v, idt = [np.ascontiguousarray(a[idx], np.float32) for a in (u, v, idt)]
    if not interval:
        return u, v, None, None
    return u, v, (idt * np.float32(0.1)).astype(np.float32), (idt * np.float32(1.9)).astype(np.float32)


def check_match(c, oracle, pr, mode_first, u, v, imin, imax):
    sf, df, good, sb, db = oracle_match(oracle, pr, mode_first, u, v, imin, imax)
    out = device_match(c, pr, mode_first, u, v, imin, imax)
    assert np.array_equal(out["status_fwd"], sf)
    assert np.array_equal(out["idepth_stereo"], df["idepth_stereo"])
    assert np.array_equal(out["idepth_min_out"], df["idepth_min_stereo"], equal_nan=True)
    assert np.array_equal(out["idepth_max_out"], df["idepth_max_stereo"], equal_nan=True)
    assert np.array_equal(out["fwd_uv"], df["lastTraceUV"])
    assert (out["status_back"][sf != 0] == 255).all() and np.array_equal(out["status_back"][good], sb)
    assert np.array_equal(out["back_uv"][good], db["lastTraceUV"])
    assert (sf == 0).mean() > 0.5 and (sb == 0).mean() > 0.5 and len(np.unique(sf)) >= 2
    return out


@pytest.mark.parametrize("interval", [False, True], ids=["fresh", "interval"])
@pytest.mark.parametrize("mode_first", [1, 0])
def test_match_bench_shape(ctx, oracle, kitti, mode_first, interval):
    check_match(ctx, oracle, kitti, mode_first, *match_case(kitti, mode_first, interval))


def test_match_small_large_small(oracle, kitti):
    """One context, three calls: the second regrows both batches of the chain (trace_reserve), the third runs on the grown ones with
    fewer points than they hold.  Sizes that are not multiples of 16 (points per workgroup of the trace) or 256."""
    rs = np.random.RandomState(71)
    c = abi.Context(0)
    try:
        c.upload_pyramid(LEFT, kitti["pyr_l"][:1]); c.upload_pyramid(RIGHT, kitti["pyr_r"][:1])
        for n, mode_first, interval in ((3001, 1, False), (19993, 0, True), (1234, 1, True)):
            idx = rs.permutation(20000)[:n]
            check_match(c, oracle, kitti, mode_first, *match_case(kitti, mode_first, interval, idx))
    finally:
        c.close()


def test_step1_end_to_end_bench_shape(ctx, oracle, kitti):
    """makeCoarseDepthL0 STEP1 (CoarseTracker.cpp:290-354) through the Python ABI at 1232x368 with 20 000 points: the points whose last
    residual is IN, rounded; the L->R->L match with the 0.1 .. 1.9 interval; the accept rule (|u - back u| < 1, 0 < depth < 50) or
    else centerProjectedTo's idepth; weight sqrtf(1e-3 / (HdiF + 1e-12)); splat frame by frame; STEP2-5.  The device chain must
    give the oracle chain's idepths and template, bit for bit."""
    pr = kitti
    n = len(pr["u"])
    rs = np.random.RandomState(7)
    cpt = np.stack([pr["u"] + rs.uniform(-1.5, 1.5, n), pr["v"] + rs.uniform(-1.5, 1.5, n),          # sub-pixel, some on shared pixels
                    pr["idepth_true"] * rs.uniform(0.8, 1.25, n)], axis=1).astype(np.float32)
    sel = np.nonzero((rs.rand(n) < 0.9) & (rs.rand(n) < 0.85))[0]          # lastResiduals[0] present and IN
    hdi = (1.0 / rs.uniform(50, 5000, n)).astype(np.float32)
    frame_of = rs.randint(0, 3, n)
    ui = (cpt[sel, 0] + np.float32(0.5)).astype(np.int32); vi = (cpt[sel, 1] + np.float32(0.5)).astype(np.int32)
    uf, vf = ui.astype(np.float32), vi.astype(np.float32)
    imin, imax = (cpt[sel, 2] * np.float32(0.1)).astype(np.float32), (cpt[sel, 2] * np.float32(1.9)).astype(np.float32)

    def accept(status_fwd, idepth_stereo, back_u):
        new_idepth = cpt[sel, 2].copy()
        good = np.nonzero(status_fwd == 0)[0]
        ids = idepth_stereo[good]
        with np.errstate(divide="ignore"):
            depth = np.float32(1.0) / ids
        ok = (np.abs(uf[good] - back_u) < 1) & (depth > 0) & (depth < 50)
        new_idepth[good[ok]] = ids[ok]
        return new_idepth, int(ok.sum())

    sf, df, good, sb, db = oracle_match(oracle, pr, 1, uf, vf, imin, imax)
    nid_o, acc_o = accept(sf, df["idepth_stereo"], db["lastTraceUV"][:, 0])
    out = device_match(ctx, pr, 1, uf, vf, imin, imax)
    nid_d, acc_d = accept(out["status_fwd"], out["idepth_stereo"], out["back_uv"][out["status_fwd"] == 0, 0])
    assert np.array_equal(nid_d, nid_o) and acc_d == acc_o
    assert 0.3 * len(sel) < acc_o < len(sel)                                # both branches of the accept rule are taken
    weight = np.sqrt((1e-3 / (hdi[sel].astype(np.float64) + 1e-12)).astype(np.float32)).astype(np.float32)
    order = np.concatenate([np.nonzero(frame_of[sel] == f)[0] for f in range(3)])
    assert crossing_groups(ui[order], vi[order], pr["w"])
    check_make_ref(ctx, oracle, 18, LEFT, pr["pyr_l"], ui[order], vi[order], nid_d[order], weight[order])


# ------------------------------------------------------------------ the benchmarked trace path
@pytest.fixture(scope="module")
def trace_case(oracle, kitti):
    """the bench's trace batch with mixed prior state: fresh points, finite intervals around the truth, intervals too narrow to
    search (SKIPPED / BADCONDITION), prior OUTLIER / OOB / GOOD statuses and prior qualities below the fresh 10000"""
    pr = kitti
    n = len(pr["u"])
    i = np.arange(n)
    rs = np.random.RandomState(81)
    col, wgt, gH, eth = _oracle_init(oracle, pr, np.ascontiguousarray(pr["pyr_l"][0]), pr["u"], pr["v"])
    idt = pr["idepth_true"].astype(np.float32)
    imin, imax = np.zeros(n, np.float32), np.full(n, np.nan, np.float32)
    wide, narrow = i % 3 == 1, i % 11 == 2
    imin[wide], imax[wide] = idt[wide] * np.float32(0.6), idt[wide] * np.float32(1.5)
    imin[narrow], imax[narrow] = idt[narrow] * np.float32(0.99), idt[narrow] * np.float32(1.01)
    prev = np.full(n, 5, np.uint8)
    prev[i % 13 == 3], prev[i % 13 == 4], prev[i % 13 == 5] = 2, 1, 0
    quality = np.full(n, 10000, np.float32)
    quality[i % 7 == 0] = rs.uniform(0.5, 5, int((i % 7 == 0).sum()))
    return dict(u=pr["u"], v=pr["v"], col=col, wgt=wgt, gH=gH, eth=eth, imin=imin, imax=imax, prev=prev, quality=quality,
                right=np.ascontiguousarray(pr["pyr_r"][0]))


def trace_points(tc, idx):
    P, d = abi.make_trace_points(len(idx), tc["u"][idx], tc["v"][idx], tc["col"][idx], tc["wgt"][idx], tc["gH"][idx], tc["eth"][idx],
                                 tc["imin"][idx], tc["imax"][idx])
    d["lastTraceStatus"][:] = tc["prev"][idx]
    d["quality"][:] = tc["quality"][idx]
    return P, d


def oracle_trace(oracle, pr, tc, idx, gn_mode):
    P, d = trace_points(tc, idx)
    st = np.zeros(len(idx), np.uint8)
    oracle.orc_trace_stereo_batch_gn(abi.fp(tc["right"]), pr["w"], pr["h"], abi.fp(pr["K32"]), pr["bl"], 1, C.byref(P), abi.bp(st), gn_mode)
    return st, d


def fetch(c, tc, idx):
    P, d = trace_points(tc, idx)
    st = np.zeros(len(idx), np.uint8)
    c.check(c.L.sdso_trace_stereo_fetch(c.h, C.byref(P), abi.bp(st)))
    return st, d


def same_trace(a, b):
    (sa, da), (sb, db) = a, b
    assert np.array_equal(sa, sb)
    for k in FIELDS:
        assert np.array_equal(da[k], db[k], equal_nan=True), k


def prepare(c, pr, tc, idx):
    P, d = trace_points(tc, idx)
    c.check(c.L.sdso_trace_stereo_prepare(c.h, RIGHT, abi.fp(pr["K32"]), pr["bl"], 1, C.byref(P)))


def fresh_ctx(pr):
    c = abi.Context(0)
    c.upload_pyramid(RIGHT, pr["pyr_r"][:1])
    return c


def test_prepared_trace_enqueues_repeat_the_input(oracle, kitti, trace_case):
    """prepare once; enqueue once, twice, three times back to back, fetching after each group: every fetch is the oracle's single
    trace and sdso_trace_stereo_batch's (an even count too: a prior OUTLIER left unrestored turns OOB, then OUTLIER again); a second
    fetch gives the same again."""
    pr, tc = kitti, trace_case
    idx = np.arange(len(tc["u"]))
    exp = oracle_trace(oracle, pr, tc, idx, 0)
    assert {0, 1, 2, 3, 4} <= set(np.unique(exp[0])) and (exp[1]["lastTraceStatus"][tc["prev"] == 2] == 1).any()   # OUTLIER -> OOB
    c = fresh_ctx(pr)
    try:
        P, d = trace_points(tc, idx)
        st = np.zeros(len(idx), np.uint8)
        c.check(c.L.sdso_trace_stereo_batch(c.h, RIGHT, abi.fp(pr["K32"]), pr["bl"], 1, C.byref(P), abi.bp(st)))
        same_trace((st, d), exp)
        prepare(c, pr, tc, idx)
        for reps in (1, 2, 3):
            for _ in range(reps):
                c.check(c.L.sdso_trace_stereo_enqueue(c.h))
            first = fetch(c, tc, idx)
            same_trace(first, exp)
        same_trace(fetch(c, tc, idx), first)
    finally:
        c.close()


def test_prepared_trace_reprepare_larger_then_smaller(oracle, kitti, trace_case):
    """prepare 20 000 points, then 31 007 (the batch grows), then 5003 (fewer than it holds), each enqueued twice: every fetch equals
    the oracle on that batch.  The later batches hold the points in another order, so stale state would show."""
    pr, tc = kitti, trace_case
    n = len(tc["u"])
    rs = np.random.RandomState(91)
    c = fresh_ctx(pr)
    try:
        for idx in (np.arange(n), np.concatenate([rs.permutation(n), rs.permutation(n)[:11007]]), rs.permutation(n)[:5003]):
            prepare(c, pr, tc, idx)
            c.check(c.L.sdso_trace_stereo_enqueue(c.h))
            c.check(c.L.sdso_trace_stereo_enqueue(c.h))
            same_trace(fetch(c, tc, idx), oracle_trace(oracle, pr, tc, idx, 0))
    finally:
        c.close()


def test_prepared_trace_gn_mode_between_enqueues(oracle, kitti, trace_case):
    """one prepared batch, the refinement mode switched between enqueues (1, 0, 1): each fetch equals the oracle's trace in the mode
    of the enqueue before it (ImmaturePoint.cpp:309-412 for 1, the DSO-native :707-769 for 0)"""
    pr, tc = kitti, trace_case
    idx = np.arange(len(tc["u"]))
    exp = {m: oracle_trace(oracle, pr, tc, idx, m) for m in (0, 1)}
    assert not np.array_equal(exp[0][1]["lastTraceUV"], exp[1][1]["lastTraceUV"])
    c = fresh_ctx(pr)
    try:
        prepare(c, pr, tc, idx)
        for mode in (1, 0, 1):
            c.check(c.L.sdso_trace_set_gn_mode(c.h, mode))
            c.check(c.L.sdso_trace_stereo_enqueue(c.h))
            same_trace(fetch(c, tc, idx), exp[mode])
    finally:
        c.L.sdso_trace_set_gn_mode(c.h, 0)
        c.close()
