"""sdso_ba_flag_points: FullSystem::removeOutliers + flagPointsForRemoval (FullSystemOptimize.cpp:1063-1084, FullSystem.cpp:965-1056)
decided on the device-resident window after sdso_ba_optimize.

Every output is an integer, so every comparison is equality: decision / counts / host_counts against tests/flag_points_ref.py applied
to the DEVICE's own post-state (sdso_ba_get_post_state), on the three windows tests/test_flag_points_ref.py vets on the CPU oracle.
The shapes: B is two full workgroups and a partial one (600 = 2 * 256 + 88), C one partial workgroup, A's residual lists are permuted by
dropResidual's swap-with-last and up to seven long.  Level-0 pyramids only, as in tests/test_ba_post_state_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import flag_points_ref as ref
import window_update_helpers as wu

pytestmark = pytest.mark.gpu

WU, WF = 33, 34


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in ref.CASES}


def _optimized(ctx, win, wid):
    wu.upload_pyramids(ctx, win)
    keep = wu.upload(ctx, win, wid)
    wu.optimize(ctx, wid)
    return wu.post_state(ctx, wid, win), keep


def _release(ctx, *wids):
    for w in wids:
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, w))


def _assert_equal(got, want, what):
    dec, cnt, hc = got
    assert np.array_equal(dec, want["decision"]), (what, np.nonzero(dec != want["decision"])[0][:10])
    assert np.array_equal(cnt, want["counts"]), (what, cnt, want["counts"])
    assert np.array_equal(hc, want["host_counts"]), what


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_decisions_equal_reference_on_device_post_state(gpu_ctx, cases, name):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases[name]
    post, keep = _optimized(ctx, win, WU)
    th = ref.median_hessian(post)
    want = ref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=th)
    got = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    print(name, "np", win["np"], "codes", got[1].tolist(), "DROP_NEGATIVE on the device:", int(got[1][ref.DROP_NEGATIVE]),
          "isOOB clauses", np.bincount(want["clause"], minlength=4)[1:].tolist(), "n >= 7", int((want["n"] >= 7).sum()))
    _assert_equal(got, want, name)
    assert got[1].sum() == win["np"]
    ref.check_coverage(name, want)
    _release(ctx, WU)


def test_null_history_equals_all_255(gpu_ctx, cases):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["A"]
    post, keep = _optimized(ctx, win, WU)
    th = ref.median_hessian(post)
    want = ref.flag_points(win, post, frame_marg, None, minIdepthH_marg=th)
    a = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, None, minIdepthH_marg=th)
    b = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, np.full(2 * win["np"], 255, np.uint8), minIdepthH_marg=th)
    _assert_equal(a, want, "NULL")
    _assert_equal(b, want, "all 255")
    # ... and the history of the other tests is not a no-op on this window
    assert (ref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=th)["decision"] != want["decision"]).sum() >= 5
    _release(ctx, WU)


def test_call_is_repeatable_and_changes_nothing(gpu_ctx, cases):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["A"]
    before, keep = _optimized(ctx, win, WU)
    th = ref.median_hessian(before)
    a = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    b = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    wu.assert_same(before, wu.post_state(ctx, WU, win), what="post-state after two sdso_ba_flag_points")
    # other settings and flags on the same window: the call keeps nothing from the one before
    fm2 = np.zeros(win["nf"], np.uint8); fm2[3] = 1
    c = ctx.flag_points(WU, win["nf"], win["np"], fm2, None, minGoodActiveResForMarg=2, minGoodResForMarg=6, minIdepthH_marg=0.5 * th)
    _assert_equal(c, ref.flag_points(win, before, fm2, None, minGoodActiveResForMarg=2, minGoodResForMarg=6, minIdepthH_marg=0.5 * th), "other settings")
    _assert_equal(ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th), dict(decision=a[0], counts=a[1], host_counts=a[2]), "again")
    _release(ctx, WU)


def test_carried_state_after_window_update(gpu_ctx, cases):
    """The keyframe's next steps on the resident window: linearizeAll(true)'s toRemove residuals and removeOutliers' points leave through
    sdso_ba_window_update, the window is optimized and flagged again — equal to a fresh upload of the edited window, and to the reference."""
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["A"]
    post, keep = _optimized(ctx, win, WU)
    th = ref.median_hessian(post)
    dec, cnt, hc = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    edit = dict(drop_res=[int(r) for r in np.nonzero(post["toRemove"])[0]], drop_point=(dec == ref.DROP_NO_RESIDUAL).astype(np.uint8))
    assert len(edit["drop_res"]) > 0 and edit["drop_point"].sum() >= 5
    w2, maps = wu.flatten(win, wu.values_from_post(win, post), edit, {})
    point_src = np.asarray(maps[1])
    assert w2["np"] == win["np"] - int(edit["drop_point"].sum()) and w2["nr"] == win["nr"] - len(edit["drop_res"])
    # lastResiduals[k].second of the survivors: what the caller had, else the state of a residual into frame nf-1-k that has just left
    gone = last_gone.reshape(-1, 2).copy()
    for k in range(2):
        sel = (post["toRemove"] == 1) & (win["res_target"] == win["nf"] - 1 - k)
        pts = win["res_point"][sel]
        fill = gone[pts, k] == 255
        gone[pts[fill], k] = post["state_state"][sel][fill]
    gone2 = np.ascontiguousarray(gone[point_src]).reshape(-1)
    assert (gone2 != last_gone.reshape(-1, 2)[point_src].reshape(-1)).sum() >= 5
    wu.upload(ctx, w2, WF)
    assert wu.update(ctx, WU, edit) == 0, ctx.L.sdso_last_error(ctx.h)
    wu.optimize(ctx, WU); wu.optimize(ctx, WF)
    pU, pF = wu.post_state(ctx, WU, w2), wu.post_state(ctx, WF, w2)
    wu.assert_same(pU, pF, what="optimize after the update")
    th2 = ref.median_hessian(pU)
    gU = ctx.flag_points(WU, w2["nf"], w2["np"], frame_marg, gone2, minIdepthH_marg=th2)
    gF = ctx.flag_points(WF, w2["nf"], w2["np"], frame_marg, gone2, minIdepthH_marg=th2)
    want = ref.flag_points(w2, pU, frame_marg, gone2, minIdepthH_marg=th2)
    print("edited window: np", w2["np"], "nr", w2["nr"], "codes", gU[1].tolist())
    _assert_equal(gU, want, "updated window")
    _assert_equal(gF, want, "fresh upload of the edited window")
    assert min(want["counts"][c] for c in (ref.KEEP, ref.MARGINALIZE, ref.DROP_WEAK, ref.DROP_NOT_INLIER)) >= 5
    _release(ctx, WU, WF)


def test_refusals_leave_the_window_usable(gpu_ctx, cases):
    ctx, L = gpu_ctx, gpu_ctx.L
    win, frame_marg, last_gone = cases["C"]
    nf, npts = win["nf"], win["np"]
    ERR_ARG, ERR_STATE = -1, -4
    dec = np.zeros(npts, np.uint8)

    def call(wid=WU, fm=frame_marg, lg=last_gone, null=None, **kw):
        F, keep = abi.make_flag_points(fm if fm is not None else np.zeros(nf, np.uint8), lg, **kw)
        if fm is None:
            F.frame_marg = None
        return L.sdso_ba_flag_points(ctx.h, wid, None if null == "struct" else C.byref(F), None if null == "decision" else abi.bp(dec), None, None)

    wu.upload_pyramids(ctx, win)
    wu.upload(ctx, win, WU)
    assert call() == ERR_STATE and b"post-state" in L.sdso_last_error(ctx.h)                    # no optimize has ended
    wu.optimize(ctx, WU)
    post = wu.post_state(ctx, WU, win)
    th = ref.median_hessian(post)
    want = ref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=th)
    good = ctx.flag_points(WU, nf, npts, frame_marg, last_gone, minIdepthH_marg=th)
    _assert_equal(good, want, "first good call")
    bad = last_gone.copy(); bad[2 * npts - 1] = 3
    assert call(lg=bad) == ERR_ARG and b"last_gone" in L.sdso_last_error(ctx.h)
    assert call(fm=None) == ERR_ARG and b"frame_marg" in L.sdso_last_error(ctx.h)
    assert call(null="struct") == ERR_ARG
    assert call(null="decision") == ERR_ARG
    assert call(minGoodResForMarg=-1) == ERR_ARG and call(minGoodActiveResForMarg=-1) == ERR_ARG and call(minIdepthH_marg=-1.0) == ERR_ARG
    assert call(wid=977) == ERR_ARG and b"unknown window" in L.sdso_last_error(ctx.h)
    _assert_equal(ctx.flag_points(WU, nf, npts, frame_marg, last_gone, minIdepthH_marg=th), want, "good call after the refusals")
    wu.assert_same(post, wu.post_state(ctx, WU, win), what="post-state after the refusals")
    # an update discards the post-state
    edit = dict(drop_res=[int(r) for r in np.nonzero(post["toRemove"])[0]], drop_point=(good[0] == ref.DROP_NO_RESIDUAL).astype(np.uint8))
    w2, maps = wu.flatten(win, wu.values_from_post(win, post), edit, {})
    assert wu.update(ctx, WU, edit) == 0, L.sdso_last_error(ctx.h)
    dec = np.zeros(w2["np"], np.uint8)
    gone2 = np.ascontiguousarray(last_gone.reshape(-1, 2)[np.asarray(maps[1])]).reshape(-1)
    assert call(lg=gone2) == ERR_STATE and b"post-state" in L.sdso_last_error(ctx.h)
    wu.optimize(ctx, WU)
    p2 = wu.post_state(ctx, WU, w2)
    th2 = ref.median_hessian(p2)
    g2 = ctx.flag_points(WU, w2["nf"], w2["np"], frame_marg, gone2, minIdepthH_marg=th2)
    _assert_equal(g2, ref.flag_points(w2, p2, frame_marg, gone2, minIdepthH_marg=th2), "good call after the update")
    # flagPointsForRemoval's marginalised points are linearised by sdso_ba_marginalize_points: the window no longer answers
    assert (g2[0] == ref.MARGINALIZE).sum() >= 5
    wu.marginalize_points(ctx, WU, w2, (g2[0] == ref.MARGINALIZE).astype(np.uint8))
    assert call(lg=gone2, minIdepthH_marg=th2) == ERR_STATE and b"linearised" in L.sdso_last_error(ctx.h)
    _release(ctx, WU)
