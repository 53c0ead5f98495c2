"""sdso_ba_window_update: an uploaded window edited in place is the window a fresh upload of the hand-flattened edit would make.

"Equal" is np.array_equal on every array; no tolerance is introduced here.  The one non-exact comparison is the oracle check that closes
the keyframe chain, with the bars of tests/test_ba_post_state_gpu.py::check_post_state (quoted there with their lines)."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import synth
import window_edit_ref as ref
import window_update_helpers as wu

pytestmark = pytest.mark.gpu

SDSO_ERR_STATE = -4
WU, WF = 3, 4                      # window ids of the two paths


@pytest.fixture(scope="module")
def win_c3():
    return synth.ba_window(w=1232, h=368, nf=8, pts_per_kf=250, seed=3001)      # configs[2]


@pytest.fixture(scope="module")
def win_small():
    return synth.ba_window(w=320, h=240, nf=3, pts_per_kf=60, seed=3107)


def _release(ctx, *wids):
    for w in wids:
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, w))


def test_fresh_upload_path_is_deterministic(gpu_ctx, win_c3):
    """The precondition of every comparison below: upload, optimize, post-state twice gives the same bits."""
    ctx, win = gpu_ctx, win_c3
    wu.upload_pyramids(ctx, win)
    runs = []
    for wid in (WU, WF):
        wu.upload(ctx, win, wid)
        wu.optimize(ctx, wid)
        runs.append(wu.post_state(ctx, wid, win))
    wu.assert_same(runs[0], runs[1], what="two fresh runs")
    _release(ctx, WU, WF)


def test_update_after_optimize_equals_fresh_upload(gpu_ctx, win_c3):
    ctx, win = gpu_ctx, wu.with_history(win_c3, 23)              # depth priors, counts, baselines, residuals that are not new: all carried
    assert win["hasDepthPrior"].sum() > 0 and (win["res_isNew"] == 0).sum() > 0
    wu.upload_pyramids(ctx, win)
    wu.upload(ctx, win, WU)
    wu.optimize(ctx, WU)
    d = wu.post_state(ctx, WU, win)
    # idepth_zero == idepth on the device after an optimize (doStepFromBackup sets both): EFPoint::deltaF, kept next to them, is zero
    dl = np.ones(win["np"], np.float32)
    ctx.check(ctx.L.sdso_ba_get_deltas(ctx.h, WU, None, None, None, abi.fp(dl)))
    assert not dl.any()
    edit = wu.outlier_edit(win, d)
    print("n_toRemove", len(edit["drop_res"]), "of", win["nr"], "points dropped", int(edit["drop_point"].sum()), "of", win["np"])
    assert len(edit["drop_res"]) > 0 and edit["drop_point"].sum() > 0
    # ---- path F, then path U
    w2, maps = wu.flatten(win, wu.values_from_post(win, d), edit, {})
    wu.upload(ctx, w2, WF)
    assert wu.update(ctx, WU, edit) == 0, ctx.L.sdso_last_error(ctx.h)
    assert wu.get_order(ctx, WU, w2["nf"], w2["np"], w2["nr"]) == tuple(list(m) for m in maps)
    P, _ = abi.make_post_state(w2["nf"], w2["np"], w2["nr"])
    assert ctx.L.sdso_ba_get_post_state(ctx.h, WU, C.byref(P)) != 0           # like a fresh upload: no post-state until the next optimize
    sU, sF = wu.snapshot(ctx, WU, w2), wu.snapshot(ctx, WF, w2)
    wu.assert_same(sU, sF, what="update vs fresh upload")
    assert sU["isActive"].sum() > 0.4 * w2["nr"]
    # the next optimize counts numGoodResiduals / maxRelBaseline over the residuals that are still new (FullSystemOptimize.cpp:64-77) on top
    # of the carried history, and the carried depth priors enter every point's Hessian
    wu.optimize(ctx, WU); wu.optimize(ctx, WF)
    pU, pF = wu.post_state(ctx, WU, w2), wu.post_state(ctx, WF, w2)
    wu.assert_same(pU, pF, what="optimize after the update")
    inc = np.bincount(w2["res_point"], weights=(pU["isActiveAndIsGoodNEW"] & w2["res_isNew"]).astype(np.float64), minlength=w2["np"]).astype(np.int32)
    assert np.array_equal(pU["numGoodResiduals"], w2["numGoodResiduals"] + inc) and (w2["res_isNew"] == 0).sum() > 0 and w2["hasDepthPrior"].sum() > 0
    flags = (np.random.RandomState(17).rand(w2["np"]) < 0.1).astype(np.uint8)
    mU, mF = wu.marginalize_points(ctx, WU, w2, flags), wu.marginalize_points(ctx, WF, w2, flags)
    for a, b, k in zip(mU, mF, ("HM", "bM", "counts")):
        assert np.array_equal(a, b), k
    assert np.abs(mU[0]).max() > 0 and mU[2][2] > 0
    _release(ctx, WU, WF)


# ------------------------------------------------------------------ a keyframe chain
CHAIN_NF, CHAIN_WIN = 11, 8


@pytest.fixture(scope="module")
def chain_problem():
    """One 11-keyframe problem; window k = its frames k .. k+7.  A seeded part of every host's points is held back ("immature") and
    enters one or two keyframes after its host did."""
    big = synth.ba_window(w=1232, h=368, nf=CHAIN_NF, pts_per_kf=110, seed=3301, max_res_per_point=10)
    rs = np.random.RandomState(41)
    first = np.maximum(big["host"] - (CHAIN_WIN - 1), 0)                       # the first window that holds the point's host
    big["enters"] = first + (rs.rand(big["np"]) < 0.35) * rs.randint(1, 3, big["np"])
    return big


def _first_window(big):
    fr = list(range(CHAIN_WIN))
    pts = np.nonzero((big["host"] < CHAIN_WIN) & (big["enters"] == 0))[0]
    pmap = -np.ones(big["np"], np.int64); pmap[pts] = np.arange(len(pts))
    rk = np.nonzero((pmap[big["res_point"]] >= 0) & (big["res_target"] < CHAIN_WIN))[0]
    w = dict(big)
    w.update(nf=CHAIN_WIN, np=len(pts), nr=len(rk))
    for k in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID"):
        w[k] = np.ascontiguousarray(big[k][fr])
    w["pyrs"] = [big["pyrs"][f] for f in fr]
    for k in ("u", "v", "idepth", "idepth_zero", "color", "weights", "host", "hasDepthPrior"):
        w[k] = np.ascontiguousarray(big[k][pts])
    w["res_point"] = pmap[big["res_point"][rk]].astype(np.int32); w["res_target"] = np.ascontiguousarray(big["res_target"][rk]); w["res_state"] = np.zeros(len(rk), np.uint8)
    n = 8 * CHAIN_WIN + 4
    w["HM"] = np.zeros((n, n)); w["bM"] = np.zeros(n)
    for k in ("enters", "idepth_true", "poses", "affs"):
        w.pop(k, None)
    return w


def _keyframe_edit(big, cur, k, marg_flags, rs):
    """window k -> window k+1 (stages 2-7): the marginalised points leave in allPointsToMarg order (window order), a seeded part of the
    others is dropped, the oldest frame leaves, frame k+8 comes, every surviving point of the two newest hosts observes it, and the
    points of the big problem that enter at keyframe k+1 are inserted with a residual into every other frame."""
    nf = cur["nf"]
    marg = [int(p) for p in np.nonzero(marg_flags)[0]]
    drop = ((rs.rand(cur["np"]) < 0.03) & (marg_flags == 0)).astype(np.uint8)
    stay = (marg_flags == 0) & (drop == 0)
    new_f = k + CHAIN_WIN                                                       # its index in the big problem (= frameID)
    add_res = [(int(p), nf) for p in np.nonzero(stay & (cur["host"] >= nf - 2))[0]]
    ent = np.nonzero((big["enters"] == k + 1) & (big["host"] > k) & (big["host"] <= new_f))[0]
    hosts = [int(big["host"][p]) - k for p in ent]                              # before-the-call numbering: big frame k is index 0
    pt_res = [(q, t) for q, h in enumerate(hosts) for t in range(1, nf + 1) if t != h]
    edit = dict(remove_points=marg, drop_point=drop, remove_frames=[0], n_add_frames=1, add_res=add_res, add_points=hosts, pt_res=pt_res)
    payload = dict(
        add_frames={key: np.ascontiguousarray(big[key][new_f:new_f + 1]) for key in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID")},
        add_points={key: np.ascontiguousarray(big[key][ent]) for key in ("u", "v", "idepth", "idepth_zero", "color", "weights", "hasDepthPrior")})
    payload["add_frames"]["pyrs"] = [big["pyrs"][new_f]]
    payload["add_points"]["hasDepthPrior"] = (rs.rand(len(ent)) < 0.2).astype(np.uint8)
    payload["add_res_isNew"] = (rs.rand(len(add_res)) < 0.8).astype(np.uint8)
    payload["pt_res_isNew"] = (rs.rand(len(pt_res)) < 0.8).astype(np.uint8)
    return edit, payload


def test_keyframe_chain_through_update_only(gpu_ctx, oracle, chain_problem):
    ctx, big = gpu_ctx, chain_problem
    rs = np.random.RandomState(97)
    cur = wu.with_history(_first_window(big), 29)
    wu.upload_pyramids(ctx, cur)
    wu.upload(ctx, cur, WU); wu.upload(ctx, cur, WF)
    resInM_F = 0
    for k in range(3):
        # ---- FullSystem::optimize
        wu.optimize(ctx, WU); wu.optimize(ctx, WF)
        dU, dF = wu.post_state(ctx, WU, cur), wu.post_state(ctx, WF, cur)
        wu.assert_same(dU, dF, skip=("resInM",), what="post-state of keyframe %d" % k)
        assert dU["resInM"][0] == resInM_F                                     # (path F starts every window at 0; path U keeps counting)
        # ---- toRemove, removeOutliers: the edit of the test above.  The prior of path F: what its window holds
        edit = wu.outlier_edit(cur, dU)
        assert len(edit["drop_res"]) > 0
        n = 8 * cur["nf"] + 4
        nxt, maps = wu.flatten(cur, wu.values_from_post(cur, dF), edit, {}, HM=cur["HM"], bM=cur["bM"])
        assert wu.update(ctx, WU, edit) == 0, ctx.L.sdso_last_error(ctx.h)
        wu.upload(ctx, nxt, WF)
        assert wu.get_order(ctx, WU, nxt["nf"], nxt["np"], nxt["nr"]) == tuple(list(m) for m in maps)
        cur = nxt
        # ---- flagPointsForRemoval + marginalizePointsF: every point of the oldest frame and a seeded part of the others
        flags = ((cur["host"] == 0) | (rs.rand(cur["np"]) < 0.05)).astype(np.uint8)
        mU, mF = wu.marginalize_points(ctx, WU, cur, flags), wu.marginalize_points(ctx, WF, cur, flags)
        assert np.array_equal(mU[0], mF[0]) and np.array_equal(mU[1], mF[1]) and np.array_equal(mU[2][:2], mF[2][:2])
        resInM_F += int(mF[2][2])
        assert mU[2][2] == resInM_F and mF[2][2] > 0
        # ---- marginalizeFrame of the oldest keyframe: the prior stays on the device in path U, path F takes the host copy
        hU, hF = wu.marginalize_frame_dev(ctx, WU, 0, cur["nf"] - 1), wu.marginalize_frame_dev(ctx, WF, 0, cur["nf"] - 1)
        assert np.array_equal(hU[0], hF[0]) and np.array_equal(hU[1], hF[1]) and np.abs(hF[0]).max() > 0
        # ---- window k -> window k+1
        edit, payload = _keyframe_edit(big, cur, k, flags, rs)
        assert len(edit["add_res"]) > 0 and len(edit["add_points"]) > 0 and edit["drop_point"].sum() > 0
        ctx.upload_pyramid(wu.SLOT0 + k + CHAIN_WIN, big["pyrs"][k + CHAIN_WIN][:1])
        HM2, bM2 = wu.zero_extend(hF[0], hF[1], n)
        nxt, maps = wu.flatten(cur, wu.values_from_state(ctx, WF, cur), edit, payload, HM=HM2, bM=bM2)
        assert wu.update(ctx, WU, edit, payload) == 0, ctx.L.sdso_last_error(ctx.h)
        wu.upload(ctx, nxt, WF)
        assert wu.get_order(ctx, WU, nxt["nf"], nxt["np"], nxt["nr"]) == tuple(list(m) for m in maps)
        assert list(nxt["frameID"]) == list(range(k + 1, k + 1 + CHAIN_WIN))
        cur = nxt
    # ---- the fourth optimize: both paths, and the oracle on the hand-flattened window (the chain cannot be self-consistent and wrong)
    W, keep = wu.make_window(cur, with_images=True)
    h = oracle.orc_ba_create(C.byref(W))
    oo = abi.BAOptResult()
    oracle.orc_ba_optimize(h, 6, None, None, None, C.byref(oo))
    Po, do = abi.make_post_state(cur["nf"], cur["np"], cur["nr"])
    oracle.orc_ba_get_post_state(h, C.byref(Po))
    oracle.orc_ba_destroy(h)
    wu.optimize(ctx, WU); wu.optimize(ctx, WF)
    dU, dF = wu.post_state(ctx, WU, cur), wu.post_state(ctx, WF, cur)
    wu.assert_same(dU, dF, skip=("resInM",), what="post-state of the last keyframe")
    flips = int((dU["state_state"] != do["state_state"]).sum())
    dist = dict(iterations=(int(dU["counts"][3]), Po.result.iterations), flips=flips, flips_bar=max(2, cur["nr"] // 2000),
                state=float(np.abs(dU["state"] - do["state"]).max()), evalPT=float(np.abs(dU["evalPT"] - do["evalPT"]).max()),
                idepth=float(np.abs(dU["idepth"] - do["idepth"]).max()))
    print("chain vs oracle (path U == path F):", dist)
    # the bars of tests/test_ba_post_state_gpu.py::check_post_state
    assert dU["counts"][3] == Po.result.iterations, dist                        # :100
    assert flips <= max(2, cur["nr"] // 2000), dist                             # :102
    assert dist["state"] <= 1e-4 and dist["evalPT"] <= 1e-4, dist               # :114-119
    assert dist["idepth"] <= 5e-5, dist                                         # :133
    _release(ctx, WU, WF)


# ------------------------------------------------------------------ small shapes and refusals
def _bits(ctx, wid, win):
    wu.optimize(ctx, wid, 4)
    return wu.post_state(ctx, wid, win)


def test_small_shapes_and_refusals(gpu_ctx, win_small):
    ctx, win = gpu_ctx, win_small
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    wu.upload_pyramids(ctx, win)
    wu.upload(ctx, win, WF)
    want = _bits(ctx, WF, win)
    # ---- the empty edit: identity maps, and the window optimises to the same bits
    wu.upload(ctx, win, WU)
    assert wu.update(ctx, WU, {}) == 0
    assert wu.get_order(ctx, WU, nf, npts, nr) == (list(range(nf)), list(range(npts)), list(range(nr)))
    wu.assert_same(_bits(ctx, WU, win), want, what="after the empty edit")
    # ---- refusals leave the window as it was.  (1) a member of a batch
    wu.upload(ctx, win, WU)
    ids = np.array([WU], np.int32)
    ctx.check(ctx.L.sdso_ba_batch_create(ctx.h, 1, abi.ip(ids)))
    assert wu.update(ctx, WU, {}) == SDSO_ERR_STATE and b"batch" in ctx.L.sdso_last_error(ctx.h)
    wu.upload(ctx, win, WU)                                                     # (dissolves the batch)
    # (2) an appended frame without a pyramid
    k = dict(evalPT=win["evalPT"][:1], state=win["state"][:1], state_zero=win["state_zero"][:1], ab_exposure=win["ab_exposure"][:1],
             frameEnergyTH=win["frameEnergyTH"][:1], frameID=np.array([977], np.int32))
    assert wu.update(ctx, WU, dict(n_add_frames=1), dict(add_frames=k)) == -1 and b"pyramid" in ctx.L.sdso_last_error(ctx.h)
    # (3) the prior rule: a frame leaves without sdso_ba_marginalize_frame_dev; with it for another frame; with it and no frame leaving
    gone0 = dict(drop_point=(win["host"] == 0).astype(np.uint8), remove_frames=[0])
    assert wu.update(ctx, WU, gone0) == SDSO_ERR_STATE and b"marginalize_frame_dev" in ctx.L.sdso_last_error(ctx.h)
    wu.marginalize_frame_dev(ctx, WU, 1, nf - 1)
    assert wu.update(ctx, WU, gone0) == SDSO_ERR_STATE
    assert wu.update(ctx, WU, {}) == SDSO_ERR_STATE and b"removes no frame" in ctx.L.sdso_last_error(ctx.h)
    # (4) a linearised survivor: marginalize_points linearises the active residuals of the flagged points, and here they all stay
    flags = np.zeros(npts, np.uint8); flags[:10] = 1
    assert wu.marginalize_points(ctx, WU, win, flags)[2][2] > 0                 # (some residual went into the prior, so some is linearised)
    other_pt = np.zeros(npts, np.uint8); other_pt[npts - 1] = 1
    assert wu.update(ctx, WU, dict(drop_point=other_pt)) == SDSO_ERR_STATE
    assert b"linearised" in ctx.L.sdso_last_error(ctx.h)
    # ... and after all these refusals the window still gives the bits of an untouched one that went through the same calls
    wu.upload(ctx, win, WF)
    wu.marginalize_frame_dev(ctx, WF, 1, nf - 1)
    wu.marginalize_points(ctx, WF, win, flags)
    wu.assert_same(_bits(ctx, WU, win), _bits(ctx, WF, win), what="after the refused calls")
    # ---- every point leaves
    wu.upload(ctx, win, WU)
    vals = wu.values_from_state(ctx, WU, win)
    assert wu.update(ctx, WU, dict(drop_point=np.ones(npts, np.uint8))) == 0
    assert wu.get_order(ctx, WU, nf, 0, 0) == (list(range(nf)), [], [])
    empty, _ = wu.flatten(win, vals, dict(drop_point=np.ones(npts, np.uint8)), {})
    wu.upload(ctx, empty, WF)
    wu.assert_same(_bits(ctx, WU, empty), _bits(ctx, WF, empty), what="the window without points")
    _release(ctx, WU, WF)


def test_second_ctx_updates_its_own_window(gpu_ctx, win_small):
    """State is per sdso_ctx: another ctx editing its window of the same id leaves this one alone."""
    ctx, win = gpu_ctx, win_small
    wu.upload_pyramids(ctx, win)
    wu.upload(ctx, win, WF)
    want = _bits(ctx, WF, win)
    wu.upload(ctx, win, WU)
    other = abi.Context(0)
    try:
        wu.upload_pyramids(other, win)
        wu.upload(other, win, WU)
        assert wu.update(other, WU, dict(drop_point=(win["host"] == 1).astype(np.uint8), drop_res=[0])) == 0
        assert ctx.L.sdso_ba_window_get_order(ctx.h, WU, None, None, None) == SDSO_ERR_STATE      # this ctx's window was never updated
        wu.assert_same(_bits(ctx, WU, win), want, what="the first ctx's window")
        o_np = int((win["host"] != 1).sum())
        fs = np.zeros(win["nf"], np.int32)
        other.check(other.L.sdso_ba_window_get_order(other.h, WU, abi.ip(fs), None, None))
        assert list(fs) == list(range(win["nf"]))
        wu.optimize(other, WU, 4)
        idp = np.zeros(o_np, np.float32)
        other.check(other.L.sdso_ba_get_state(other.h, WU, None, abi.fp(idp), None))
        assert np.isfinite(idp).all()
    finally:
        other.close()
    _release(ctx, WU, WF)
