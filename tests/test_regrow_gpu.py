"""Growth of a ctx's own work buffers (csrc/devbuf.h) leaves results untouched.  For five entry points one fresh context runs a small
problem, then one large enough to pass every slack formula of the buffers it uses (64 and 1024 points: n + n / 4 + 64, n + n / 2 + 8,
bytes + bytes / 2 + 4096 and the exact sizes are all outgrown; or a second image size where the image sizes the buffer), then the small
one again.  Each of the three results must be bit-identical to the same call on a context that has seen nothing else: a buffer that was
freed and allocated anew, a view left pointing into the old block, or a stride that did not follow its buffer would all show here.

Shapes: 320x240, the smallest the smoke runs of these generators use; the selector's images are the smallest with three pyramid levels
and one 32x32 cell.  Two contexts of this module's own are alive at most, one after the other."""
import ctypes as C

import numpy as np
import pytest

import distmap_cases as DC
import helpers
from sdso_amd import abi
import synth
import window_update_helpers as wu

pytestmark = pytest.mark.gpu
W, H = 320, 240
SMALL, LARGE = 64, 1024
f32 = np.float32


def _fresh(run):
    ctx = abi.Context(0)
    try:
        return run(ctx)
    finally:
        ctx.close()


def _same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)


def _check_sequence(small, large):
    """small, large, small on one context against each of them alone on a fresh one"""
    alone = [_fresh(small), _fresh(large)]
    ctx = abi.Context(0)
    try:
        for step, (run, want) in enumerate(((small, alone[0]), (large, alone[1]), (small, alone[0]))):
            _same_bits(run(ctx), want, "step %d" % step)
    finally:
        ctx.close()
    assert any(not np.array_equal(a, 0 * a) for a in alone[0]) and any(not np.array_equal(a, 0 * a) for a in alone[1])   # (something was computed)


# ------------------------------------------------------------------ traceStereo
@pytest.fixture(scope="module")
def pair():
    return synth.stereo_problem(w=W, h=H, npts=LARGE, seed=4031)


def _trace(pr, n):
    left, right = np.ascontiguousarray(pr["pyr_l"][0]), np.ascontiguousarray(pr["pyr_r"][0])
    u, v = np.ascontiguousarray(pr["u"][:n]), np.ascontiguousarray(pr["v"][:n])
    K, bl = np.array(pr["K"], f32), float(pr["calib"]["baseline"])

    def run(ctx):
        ctx.upload_pyramid(80, [left]); ctx.upload_pyramid(81, [right])
        col, wgt, gH, eth = np.zeros((n, 8), f32), np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros(n, f32)
        ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, 80, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
        P, d = abi.make_trace_points(n, u, v, col, wgt, gH, eth)
        st = np.zeros(n, np.uint8)
        ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, 81, abi.fp(K), bl, 1, C.byref(P), abi.bp(st)))
        assert (st == 0).sum() > n // 8                        # IPS_GOOD: the search ran
        return [st, col, wgt, gH, eth] + [d[k] for k in ("idepth_min_stereo", "idepth_max_stereo", "idepth_stereo", "quality", "lastTraceStatus", "lastTraceUV",
                                                         "lastTracePixelInterval")]
    return run


def test_trace_stereo_batch(pair):
    assert len(pair["u"]) == LARGE
    _check_sequence(_trace(pair, SMALL), _trace(pair, LARGE))


# ------------------------------------------------------------------ the coarse tracker's evaluation batch
@pytest.fixture(scope="module")
def track():
    return synth.tracker_problem(w=W, h=H, npts=LARGE, seed=2001)


def _eval_batch(prob, npts, nprob):
    """nprob evaluations over the levels of a template cut to npts points per level"""
    pc = [{k: p[k][:npts] for k in ("u", "v", "idepth", "color")} for p in prob["pc"]]
    assert all(len(p["u"]) == npts for p in pc)
    prm = helpers.track_params(prob)
    rs = np.random.RandomState(4)
    L = abi.load()
    evs = []
    for i in range(nprob):
        T = synth.se3_exp(np.array([0.02, -0.01, 0.35, 0.004, -0.006, 0.002]) + rs.normal(0, 3e-3, 6))
        ev = abi.TrackEval()
        L.sdso_track_make_eval(C.byref(prm), i % prob["levels"], C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(0.01, 0.5)), 1.0, C.byref(ev))
        evs.append(ev)
    arr = (abi.TrackEval * nprob)(*evs)
    refs, frames = np.full(nprob, 1, np.int32), np.full(nprob, 2, np.int32)

    def run(ctx):
        ctx.upload_pyramid(2, prob["pyr_new"])
        ctx.set_ref(1, pc)
        Hs, b, res, nw = np.zeros((nprob, 64)), np.zeros((nprob, 8)), np.zeros((nprob, 6)), np.zeros(nprob, np.int32)
        ctx.check(ctx.L.sdso_track_calc_res_gs_batch(ctx.h, nprob, abi.ip(refs), abi.ip(frames), arr, abi.dp(Hs), abi.dp(b), abi.dp(res), abi.ip(nw)))
        assert nw.min() > 0
        return [Hs, b, res, nw]
    return run


def test_tracker_evaluation_batch(track):
    # 2 problems of one workgroup each, then 24 of four: past nprob + nprob / 2 + 8 = 11 problems and need + need / 2 + 64 = 67 partial blocks
    _check_sequence(_eval_batch(track, SMALL, 2), _eval_batch(track, LARGE, 24))


# ------------------------------------------------------------------ windows: the distance map and the map
@pytest.fixture(scope="module")
def windows():
    return dict(small=synth.ba_window(w=W, h=H, nf=4, pts_per_kf=SMALL // 4, seed=4107), large=synth.ba_window(w=W, h=H, nf=4, pts_per_kf=LARGE // 4, seed=4108),
                wider=synth.ba_window(w=352, h=256, nf=4, pts_per_kf=SMALL // 4, seed=4109))


def _geoms(win):
    """the window's four frames into a fifth pose a little further on (any float values do: the results are compared with themselves)"""
    e5 = np.array(win["evalPT"][-1], np.float64).copy()
    e5[11] -= 0.3
    return DC.window_geoms(np.concatenate([np.asarray(win["evalPT"], np.float64), e5[None]]), tuple(float(x) for x in win["calib_value_scaled"]))


def _distmap(win, wid):
    w, h = win["pyrs"][0][0].shape[1], win["pyrs"][0][0].shape[0]
    KRKi, Kt = _geoms(win)

    def run(ctx):
        wu.upload_pyramids(ctx, win)
        wu.upload(ctx, win, wid)
        rc, n = ctx.distmap_make_from_window(wid, w, h, KRKi, Kt)
        assert rc == 0, ctx.L.sdso_last_error(ctx.h)
        assert 0 < n <= win["np"]
        m = DC.dm_get(ctx, w, h)
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, wid))
        return [np.array([n]), m]
    return run


def test_distmap_make_from_window_on_two_image_sizes(windows):
    assert windows["small"]["np"] == SMALL
    _check_sequence(_distmap(windows["small"], 16), _distmap(windows["wider"], 17))


def _map(win, wid):
    fids = [int(f) for f in win["frameID"]]

    def run(ctx):
        wu.upload_pyramids(ctx, win)
        wu.upload(ctx, win, wid)
        wu.optimize(ctx, wid)
        post = wu.post_state(ctx, wid, win)
        ctx.map_update(wid, None, [], [])                      # every point of the window is active: the active lists are replaced
        lists = [ctx.map_get(f, 1) for f in fids]
        assert sum(len(l) for l in lists) == win["np"]
        got = ctx.map_cloud(fids, post["calib_value_scaled"].astype(f32), mode=0)
        assert got["n"] > 0
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, wid))
        return lists + [np.array([ctx.map_counts(f) for f in fids]), got["xyz"], got["rgb"], got["first"], got["kept"]]
    return run


def test_map_update_and_cloud(windows):
    # the same keyframes all through: 16, then 256, then 16 active points each (a list keeps its block of 64 records until it is outgrown)
    assert windows["large"]["np"] == LARGE and np.array_equal(windows["large"]["frameID"], windows["small"]["frameID"])
    _check_sequence(_map(windows["small"], 35), _map(windows["large"], 35))


# ------------------------------------------------------------------ the pixel selector
def _select(w, h, seed):
    pyr = synth.tracker_problem(w=w, h=h, npts=50, seed=seed)["pyr_ref"]
    assert len(pyr) >= 3 and w >= 32 and h >= 32

    def run(ctx):
        ctx.upload_pyramid(91, pyr)
        m, pot, num = np.zeros((h, w), f32), C.c_int(3), C.c_int(0)
        ctx.check(ctx.L.sdso_pixel_select(ctx.h, 91, 150.0, 1, 1.0, C.byref(pot), abi.fp(m), C.byref(num)))
        assert num.value == int((m != 0).sum()) > 20
        return [m, np.array([pot.value, num.value])]
    return run


def test_pixel_select_on_two_image_sizes():
    # a change of size, not only a growth: the random pattern and the kept map are made anew both ways
    _check_sequence(_select(160, 128, 7), _select(192, 128, 8))
