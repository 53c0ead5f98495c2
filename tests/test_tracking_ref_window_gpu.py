"""sdso_track_make_ref_from_window: CoarseTracker::setCoarseTrackingRef -> makeCoarseDepthL0 (CoarseTracker.cpp:275-534, :807-826) from
the device-resident BA window, against the route it replaces (sdso_ba_get_post_state, the gather on the host, sdso_stereo_match_batch,
the accept rule, sdso_track_make_ref) — every record and every float of every template level by bit pattern: both routes run the same
kernels on the same inputs, and the new gather evaluates centerProjectedTo and the weight with the expressions of the old one.

Windows (tests/tracking_ref_window_cases.py): 320x240, 4 keyframes x 200 points and 8 x 60 (targets up to 7 in the nibbles of p_order),
residual lists permuted by dropResidual, idepth noise 0.2 so that the closing linearizeAll(true) leaves OUTLIER / toRemove residuals;
optimised for 3 iterations."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth
import tracking_ref_window_cases as TC
from tracking_ref_window_ref import expected_points

pytestmark = pytest.mark.gpu

SHAPES = {"nf4": dict(nf=4, pts_per_kf=200, seed=3101), "nf8": dict(nf=8, pts_per_kf=60, seed=3102)}
WIN = {"nf4": 71, "nf8": 72}
SLOT0 = {"nf4": 700, "nf8": 720}
REF_HOST = {"nf4": 71, "nf8": 72}          # the host route's templates
REF_NEW = 75
ERR_ARG, ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def windows(ctx):
    """per shape: the case, its upload, the post-state after 3 iterations and the host route's result (computed once, left unchanged)"""
    out = {}
    for name, spec in SHAPES.items():
        case = TC.make_case(**spec)
        up = TC.upload(ctx, case, WIN[name], SLOT0[name])
        TC.optimize(ctx, up["wid"], 3)
        post = TC.post_state(ctx, case, up["wid"])
        g, pcn = TC.host_route(ctx, case, up, REF_HOST[name], post=post)
        out[name] = dict(case=case, up=up, post=post, host=g, pcn=pcn, levels=TC.get_ref(ctx, REF_HOST[name], case["levels"]))
    return out


def same_levels(a, b):
    return all(len(x["u"]) == len(y["u"]) and all(np.array_equal(TC.bits(x[k]), TC.bits(y[k])) for k in TC.KEYS) for x, y in zip(a, b))


def check_equals_host(ctx, W, ref_slot, d, pcn):
    g, case = W["host"], W["case"]
    assert np.array_equal(d["point"], g["point"])
    for k in ("u", "v", "status_fwd", "status_back"):
        assert np.array_equal(d[k], g[k]), k
    for k in ("cpt2", "new_idepth", "weight"):
        assert np.array_equal(TC.bits(d[k]), TC.bits(g[k])), k
    assert np.array_equal(pcn[:case["levels"]], W["pcn"][:case["levels"]])
    got = TC.get_ref(ctx, ref_slot, case["levels"])
    for l in range(case["levels"]):
        assert len(got[l]["u"]) == pcn[l] == len(W["levels"][l]["u"]), l
        for k in TC.KEYS:
            assert np.array_equal(TC.bits(got[l][k]), TC.bits(W["levels"][l][k])), (l, k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_same_as_the_host_route_bit_for_bit(ctx, windows, name):
    W = windows[name]
    case, post = W["case"], W["post"]
    newest = case["res_target"] == case["nf"] - 1
    want = expected_points(post["state_state"], post["isActiveAndIsGoodNEW"], case["res_target"], case["res_point"], case["nf"] - 1, None, case["np"])
    miss = 1.0 - len(want) / newest.sum()
    assert 0.05 <= miss <= 0.60, (len(want), int(newest.sum()))
    if name == "nf8":
        assert (case["res_target"][newest.nonzero()[0]] == 7).all() and case["nf"] == 8
    d, pcn, n_border = TC.window_route(ctx, W["up"], REF_NEW)
    assert np.array_equal(d["point"], want) and len(want) > 100
    assert n_border == 0
    check_equals_host(ctx, W, REF_NEW, d, pcn)
    took = int((TC.bits(d["new_idepth"]) != TC.bits(d["cpt2"])).sum())
    assert 0.3 * len(want) < W["host"]["n_stereo"] < len(want) and took > 0.3 * len(want), \
        "stereo idepth accepted for %d of %d points (%d changed the idepth), centerProjectedTo's kept for %d" % (
            W["host"]["n_stereo"], len(want), took, len(want) - W["host"]["n_stereo"])
    assert (d["status_fwd"] != 0).any() and (d["status_back"][d["status_fwd"] != 0] == 255).all()


def test_without_outputs_the_next_reader_sees_the_template(ctx, windows):
    """n_points_out = n_border_out = pc_n_out = NULL: the call only enqueues; sdso_track_get_ref then reads the finished template"""
    W = windows["nf4"]
    rc, _, _, _ = TC.window_call(ctx, W["up"], REF_NEW + 1, want=False)
    ctx.check(rc)
    assert same_levels(TC.get_ref(ctx, REF_NEW + 1, W["case"]["levels"]), W["levels"])
    assert np.array_equal(TC.ref_points(ctx, REF_NEW + 1)["point"], W["host"]["point"])


def test_order_is_honoured(ctx):
    """Three points on one pixel: STEP1's += (CoarseTracker.cpp:352-354) depends on the order from three summands on."""
    case = TC.with_triples(TC.make_case(**SHAPES["nf4"]))
    up = TC.upload(ctx, case, 73, 740)
    TC.optimize(ctx, up["wid"], 3)
    post = TC.post_state(ctx, case, up["wid"])
    fwd, _ = TC.host_route(ctx, case, up, 81, post=post)
    assert sum(len(g) >= 3 for g in helpers.pixel_groups(fwd["u"], fwd["v"], case["w"])) >= 20
    r = slice(None, None, -1)
    pyr = case["pyrs"][-1]
    a = synth.make_pc(fwd["u"], fwd["v"], fwd["new_idepth"], fwd["weight"], pyr)
    b = synth.make_pc(fwd["u"][r], fwd["v"][r], fwd["new_idepth"][r], fwd["weight"][r], pyr)
    assert not np.array_equal(TC.bits(a[0]["idepth"]), TC.bits(b[0]["idepth"]))           # the case is sensitive to the order
    lv_fwd = TC.get_ref(ctx, 81, case["levels"])
    assert np.array_equal(TC.bits(lv_fwd[0]["idepth"]), TC.bits(a[0]["idepth"]))
    rev = np.arange(case["np"], dtype=np.int32)[::-1]
    hrev, _ = TC.host_route(ctx, case, up, 82, order=rev, post=post)
    lv_hrev = TC.get_ref(ctx, 82, case["levels"])
    assert np.array_equal(TC.bits(lv_hrev[0]["idepth"]), TC.bits(b[0]["idepth"]))
    d_rev, _, _ = TC.window_route(ctx, up, 83, order=rev)
    assert np.array_equal(d_rev["point"], hrev["point"]) and np.array_equal(d_rev["point"], fwd["point"][r])
    assert np.array_equal(TC.bits(d_rev["new_idepth"]), TC.bits(hrev["new_idepth"]))
    lv_rev = TC.get_ref(ctx, 83, case["levels"])
    assert same_levels(lv_rev, lv_hrev)
    d_fwd, _, _ = TC.window_route(ctx, up, 84)
    lv_win = TC.get_ref(ctx, 84, case["levels"])
    assert same_levels(lv_win, lv_fwd)
    assert not same_levels(lv_win[:1], lv_rev[:1])                                          # ... and the device honours it
    # a caller's order that leaves points out and is no reversal: a shuffle of the points of every second host
    sub = np.random.RandomState(3).permutation(np.nonzero(case["host"] % 2 == 0)[0]).astype(np.int32)
    hsub, _ = TC.host_route(ctx, case, up, 82, order=sub, post=post)
    d_sub, _, _ = TC.window_route(ctx, up, 83, order=sub)
    assert np.array_equal(d_sub["point"], hsub["point"]) and 0 < len(hsub["point"]) < len(fwd["point"])
    assert same_levels(TC.get_ref(ctx, 83, case["levels"]), TC.get_ref(ctx, 82, case["levels"]))
    ctx.check(ctx.L.sdso_ba_release_window(ctx.h, 73))


def test_refusals(ctx, windows):
    W = windows["nf4"]
    case, up = W["case"], W["up"]

    def valid_call_still_right():
        d, pcn, nb = TC.window_route(ctx, up, REF_NEW)
        check_equals_host(ctx, W, REF_NEW, d, pcn)

    def refused(code, **kw):
        u2 = dict(up, **{k: v for k, v in kw.items() if k in ("wid",)})
        rc, _, _, _ = TC.window_call(ctx, u2, REF_NEW, order=kw.get("order"), right=kw.get("right"))
        assert rc == code, (rc, kw.keys())
        assert ctx.L.sdso_last_error(ctx.h)
        valid_call_still_right()

    # before optimize
    W2, keep2 = abi.make_ba_window(case, frame_slots=[SLOT0["nf4"] + f for f in range(case["nf"])], dI_list=[p[0] for p in case["pyrs"]])
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, 74, C.byref(W2)))
    refused(ERR_STATE, wid=74)
    # after a sdso_ba_window_update: the post-state is gone
    TC.optimize(ctx, 74, 3)
    rc, n_before, _, _ = TC.window_call(ctx, dict(up, wid=74), REF_NEW + 2)
    assert rc == 0 and n_before == len(W["host"]["point"])
    E, keepE = abi.make_window_edit(drop_res=[0])
    ctx.check(ctx.L.sdso_ba_window_update(ctx.h, 74, C.byref(E)))
    refused(ERR_STATE, wid=74)
    ctx.check(ctx.L.sdso_ba_release_window(ctx.h, 74))
    # a right pyramid of another size, an unknown right slot, an unknown window
    small = synth.make_pyramid(np.zeros((120, 160), np.float32) + 7, 3)
    ctx.upload_pyramid(760, small)
    refused(ERR_ARG, right=760)
    refused(ERR_ARG, right=761)
    refused(ERR_ARG, wid=79)
    # point_order: a duplicate, an entry out of range
    order = np.arange(case["np"], dtype=np.int32)
    dup = order.copy(); dup[5] = dup[400]
    refused(ERR_ARG, order=dup)
    oob = order.copy(); oob[-1] = case["np"]
    refused(ERR_ARG, order=oob)
    neg = order.copy(); neg[0] = -1
    refused(ERR_ARG, order=neg)


def test_tracking_on_it(ctx, windows):
    """sdso_track_newest_coarse against the reference the new call built == against the host route's, bit for bit.  The tracked frame
    is the keyframe before the newest (same scene, a known pose)."""
    W = windows["nf4"]
    case, up = W["case"], W["up"]
    d, pcn, _ = TC.window_route(ctx, up, REF_NEW)
    fxs, fys, cxs, cys = synth.level_intrinsics(*W["post"]["K32"], case["levels"])
    prob = dict(levels=case["levels"], pyr_ref=case["pyrs"][-1], fx=fxs, fy=fys, cx=cxs, cy=cys)
    prm = helpers.track_params(prob)
    new_slot = SLOT0["nf4"] + case["nf"] - 2
    res = []
    for ref in (REF_NEW, REF_HOST["nf4"]):
        T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
        ctx.check(ctx.L.sdso_track_newest_coarse(ctx.h, ref, new_slot, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
        res.append((T.Rt(), aff.a, aff.b, out.good, out.evaluations, list(out.iterations), np.array(out.lastResiduals[:]), int(out.point_evals)))
    (R0, t0), (R1, t1) = res[0][0], res[1][0]
    assert np.array_equal(R0, R1) and np.array_equal(t0, t1)
    assert res[0][1:6] == res[1][1:6] and res[0][7] == res[1][7] > 0
    assert np.array_equal(res[0][6], res[1][6], equal_nan=True) and res[0][4] > 0
