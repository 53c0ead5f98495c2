"""The device-resident map: sdso_map_update (setFromKF's records, gathered from the resident BA window in the caller's list orders) and
sdso_map_cloud (KeyFrameDisplay::refreshPC for up to 8 keyframes), IOWrapper/Pangolin/KeyFrameDisplay.cpp:85-165, :174-295.

Every output is copied or produced by a stated sequence of IEEE operations, so every comparison is of bit patterns and bytes against
tests/map_ref.py, with no tolerance; a NaN vertex compares as "NaN in the same place".  The windows are the three of
tests/flag_points_ref.py, which tests/test_map_ref.py vets on the CPU oracle (320, 600 and 240 points: B is nine full waves and a partial
one); the hand-made lists are the smallest shapes at which the ordered compaction can go wrong."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import flag_points_ref as fref
import map_ref as ref
import window_update_helpers as wu

pytestmark = pytest.mark.gpu

WU = 35
ERR_ARG, ERR_STATE = -1, -4
F = np.float32


@pytest.fixture(scope="module")
def cases():
    return {name: fref.make_case(name) for name in ref.CASES}


def _err(ctx):
    return ctx.L.sdso_last_error(ctx.h)


def _optimized(ctx, win, wid):
    ctx.check(ctx.L.sdso_map_clear(ctx.h))
    wu.upload_pyramids(ctx, win)
    keep = wu.upload(ctx, win, wid)
    wu.optimize(ctx, wid)
    return wu.post_state(ctx, wid, win), keep


def _flag_and_update(ctx, wid, win, post, frame_marg, last_gone, lists=None, before=None):
    """sdso_ba_flag_points, map_ref's walking loops on `lists` (default: the seeded permutation), sdso_map_update -> (decision, walk, the lists
    the map must hold now)"""
    dec, _, _ = ctx.flag_points(wid, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=fref.median_hessian(post))
    w = ref.walk(lists if lists is not None else ref.point_lists(win["host"], win["nf"]), dec)
    ctx.map_update(wid, np.array([p for l in w["active"] for p in l], np.int32), w["gone"], w["gone_list"])
    return dec, w, ref.lists_after(win, post, w, before)


def _assert_lists(ctx, want, what):
    for fid, lists in want.items():
        assert ctx.map_counts(fid).tolist() == [len(lists[l]) for l in (1, 2, 3)], (what, fid)
        for l in (1, 2, 3):
            got = ctx.map_get(fid, l)
            assert np.array_equal(got.view(np.uint32), lists[l].view(np.uint32)), (what, fid, l, np.argwhere(got.view(np.uint32) != lists[l].view(np.uint32))[:5])


def _frames(win, lists):
    return [dict(lists=lists[int(f)]) for f in win["frameID"]]


def _release(ctx, *wids):
    for w in wids:
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, w))
    ctx.check(ctx.L.sdso_map_clear(ctx.h))


# ------------------------------------------------------------------ the three windows
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_records_and_camera_frame_cloud(gpu_ctx, cases, name):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases[name]
    post, keep = _optimized(ctx, win, WU)
    dec, w, lists = _flag_and_update(ctx, WU, win, post, frame_marg, last_gone)
    # ---- records: every list equals the records built from the device's own post-state, in the walked order
    act = [p for l in w["active"] for p in l]
    assert act != sorted(act) and len(w["gone"]) >= 50 and (w["gone_list"] == 2).sum() >= 5 and (w["gone_list"] == 3).sum() >= 5
    _assert_lists(ctx, lists, name)
    # ---- cloud, camera frame, the quantile thresholds (every clause decides: asserted below on the device's values too)
    fids = [int(f) for f in win["frameID"]]
    frames = _frames(win, lists)
    K4 = post["calib_value_scaled"].astype(F)
    th = ref.quantile_thresholds(frames)
    for mode in (0, 1, 2, 3):
        want = ref.cloud(frames, K4, mode=mode, **th)
        got = ctx.map_cloud(fids, K4, mode=mode, **th)
        print(name, "mode", mode, "vertices", got["n"], "kept per status", got["kept"].sum(0).tolist())
        ref.assert_cloud_equal(got, want, (name, mode))
        if mode == 1:
            dropped = [int((want["clause"] == k).sum()) for k in (1, 3, 4, 5)]
            print(name, "dropped (mode / scaled / abs / bs)", dropped, "kept", int((want["clause"] == 0).sum()))
            assert min(dropped) >= 5 and (want["clause"] == 0).sum() >= 50
        if mode == 3:
            assert got["n"] == 0 and (got["xyz"] == -77).all() and (got["rgb"] == 77).all()      # nothing written
    # ---- a single frame, and the frames in reverse order
    k = 1
    ref.assert_cloud_equal(ctx.map_cloud(fids[k:k + 1], K4, mode=0, **th), ref.cloud(frames[k:k + 1], K4, mode=0, **th), (name, "one frame"))
    ref.assert_cloud_equal(ctx.map_cloud(fids[::-1], K4, mode=1, **th), ref.cloud(frames[::-1], K4, mode=1, **th), (name, "reversed"))
    _release(ctx, WU)


def test_two_keyframes_append_and_replace(gpu_ctx, cases):
    """The flow of test_carried_state_after_window_update: update the map, edit the window (every point that left goes), optimize, flag,
    update the map again: marginalised and out lists are appended to in order, the active lists are replaced."""
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["A"]
    post, keep = _optimized(ctx, win, WU)
    dec, w1, lists1 = _flag_and_update(ctx, WU, win, post, frame_marg, last_gone)
    _assert_lists(ctx, lists1, "first keyframe")
    edit = dict(drop_res=[int(r) for r in np.nonzero(post["toRemove"])[0]], drop_point=(dec != fref.KEEP).astype(np.uint8))
    w2, maps = wu.flatten(win, wu.values_from_post(win, post), edit, {})
    point_src = np.asarray(maps[1])
    assert w2["np"] == int((dec == fref.KEEP).sum()) >= 100
    new_of_old = {int(o): n for n, o in enumerate(point_src)}
    ph2 = [[new_of_old[p] for p in l] for l in w1["active"]]                       # fh->pointHessians as the first walk left them
    gone2 = np.ascontiguousarray(last_gone.reshape(-1, 2)[point_src]).reshape(-1)
    assert wu.update(ctx, WU, edit) == 0, _err(ctx)
    assert ctx.map_update_raw(WU, None, [], []) == ERR_STATE and b"post-state" in _err(ctx)      # the edit discarded it
    _assert_lists(ctx, lists1, "after the refused update")
    wu.optimize(ctx, WU)
    post2 = wu.post_state(ctx, WU, w2)
    fm2 = np.zeros(win["nf"], np.uint8); fm2[1] = 1
    dec2, wk2, lists2 = _flag_and_update(ctx, WU, w2, post2, fm2, gone2, lists=ph2, before=lists1)
    print("second keyframe: np", w2["np"], "codes", np.bincount(dec2, minlength=6).tolist())
    assert (wk2["gone_list"] == 2).sum() >= 3 and (wk2["gone_list"] == 3).sum() >= 3 and sum(len(l) for l in wk2["active"]) >= 20
    _assert_lists(ctx, lists2, "second keyframe")
    for fid in lists1:                                                             # appended to, in order; replaced
        for l in (2, 3):
            assert np.array_equal(lists2[fid][l][:len(lists1[fid][l])], lists1[fid][l])
        assert len(lists2[fid][1]) <= len(lists1[fid][1])
    assert sum(len(lists2[f][l]) - len(lists1[f][l]) for f in lists1 for l in (2, 3)) == len(wk2["gone"])
    assert any(len(lists2[f][1]) and not np.array_equal(lists2[f][1][:, 2], lists1[f][1][:len(lists2[f][1]), 2]) for f in lists1)
    frames = _frames(win, lists2)
    K4 = post2["calib_value_scaled"].astype(F)
    th = ref.quantile_thresholds(frames)
    for mode in (0, 1):
        ref.assert_cloud_equal(ctx.map_cloud([int(f) for f in win["frameID"]], K4, mode=mode, **th), ref.cloud(frames, K4, mode=mode, **th), mode)
    _release(ctx, WU)


# ------------------------------------------------------------------ hand-made lists
K_HAND = (500.0, 510.0, 320.5, 240.25)
IMM_ID = 9100


def _records(n, seed, keep):
    """n records whose only failing clause is the baseline one (minBS = 0.5): keep[i] decides"""
    rs = np.random.RandomState(seed)
    r = np.zeros((n, ref.REC), F)
    r[:, 0] = rs.uniform(4, 600, n); r[:, 1] = rs.uniform(4, 400, n)
    r[:, 2] = rs.uniform(0.05, 2.0, n); r[:, 3] = rs.uniform(50, 1e6, n)
    r[:, 4] = np.where(np.asarray(keep, bool), 1.0, 0.25)
    r[:, 5:13] = rs.uniform(0, 255, (n, 8))
    r[:, 13:] = rs.uniform(-1, 1, (n, 3))                                          # the padding travels with a put record and decides nothing
    return r


def _special_records():
    r = _records(65, 5, np.ones(65))
    r[3, 2] = -0.3; r[7, 2] = 0.0; r[11, 2] = 1e-30; r[12, 2] = -0.0              # negative; depth inf; depth^4 overflows; -0
    r[20, 3] = 0.0; r[21, 3] = np.inf; r[22, 3] = np.nan                           # idepth_hessian 0 (var 100), inf (var 0), NaN (passes)
    r[30, 5:13] = [0, 255.9, np.nan, 256, -1, 1e10, 300.7, 0.99]
    r[31, 4] = np.nan; r[32, 2] = np.nan                                           # NaN baseline passes; NaN idepth passes and gives NaN vertices
    return r


def _imm_group(n, seed):
    rs = np.random.RandomState(seed)
    S = dict(u=rs.uniform(4, 600, n), v=rs.uniform(4, 400, n), my_type=np.ones(n), idepth_min=rs.uniform(0.01, 0.5, n),
             idepth_max=rs.uniform(0.5, 1.5, n), quality=np.full(n, 3.0), color=rs.uniform(0, 255, (n, 8)), weights=np.ones((n, 8)),
             gradH=np.ones((n, 4)), energyTH=np.full(n, 100.0), lastTraceStatus=np.zeros(n, np.uint8), lastTraceUV=np.zeros((n, 2)),
             lastTracePixelInterval=np.zeros(n))
    S = {k: np.ascontiguousarray(v, np.uint8 if k == "lastTraceStatus" else F) for k, v in S.items()}
    S["idepth_max"][::3] = np.nan                                                  # ImmaturePoint.cpp:34: not traced yet
    S["idepth_min"][::3] = 0
    return S


@pytest.fixture()
def hand_made(gpu_ctx):
    """Four keyframes through sdso_map_put, sizes 0, 1, 63, 64, 65 and 257, an empty keyframe between non-empty ones, keep patterns all /
    none / alternating / only the last lane of a wave, and an immature group through sdso_imm_put_host"""
    ctx = gpu_ctx
    ctx.check(ctx.L.sdso_map_clear(ctx.h))
    last64 = np.zeros(64); last64[63] = 1
    last257 = np.zeros(257); last257[63] = last257[127] = last257[256] = 1
    lists = {10: {1: _records(257, 1, np.arange(257) % 2), 2: _records(63, 2, np.ones(63)), 3: _records(1, 3, [1])},
             11: {1: _records(0, 0, []), 2: _records(0, 0, []), 3: _records(0, 0, [])},
             12: {1: _records(64, 4, last64), 2: _records(65, 6, np.zeros(65)), 3: _records(0, 0, [])},
             13: {1: _special_records(), 2: _records(257, 7, last257), 3: _records(64, 8, np.ones(64))}}
    for fid, l in lists.items():
        for k, r in l.items():
            ctx.map_put(fid, k, r)
    S = _imm_group(70, 9)
    ctx.L.sdso_imm_release_host(ctx.h, IMM_ID)
    ctx.imm_put(IMM_ID, S, 640, 480)
    imm = ref.immature_records(S["u"], S["v"], S["idepth_min"], S["idepth_max"], S["color"])
    yield lists, imm
    ctx.check(ctx.L.sdso_imm_release_host(ctx.h, IMM_ID))
    ctx.check(ctx.L.sdso_map_clear(ctx.h))


def test_hand_made_lists(gpu_ctx, hand_made):
    ctx = gpu_ctx
    lists, imm = hand_made
    _assert_lists(ctx, lists, "put / get")
    fids = [10, 11, 12, 13]
    imm_ids = [-1, -1, IMM_ID, -1]
    frames = [dict(lists=lists[f], imm=imm if i >= 0 else None) for f, i in zip(fids, imm_ids)]
    th = dict(scaledTH=1e30, absTH=1.0, minBS=0.5)
    for mode in (0, 1, 2):
        want = ref.cloud(frames, K_HAND, mode=mode, **th)
        got = ctx.map_cloud(fids, K_HAND, mode=mode, imm_host_id=imm_ids, **th)
        print("mode", mode, "kept", got["kept"].tolist())
        ref.assert_cloud_equal(got, want, ("hand-made", mode))
    want = ref.cloud(frames, K_HAND, mode=0, **th)
    assert want["kept"].tolist() == [[0, 128, 63, 1], [0, 0, 0, 0], [0, 1, 0, 0], [0, 60, 3, 64]]   # (the 70 immature points fail minBS = 0.5)
    assert want["first"].tolist() == [0, 8 * 192, 8 * 192, 8 * 193, 8 * 320]
    assert np.isnan(want["xyz"]).any()                                              # the record with a NaN idepth
    # ---- the immature group at minBS = 0 in mode 0: the untraced points emit NaN vertices; at minBS > 0 (above) none is emitted
    th0 = dict(scaledTH=1e30, absTH=1.0, minBS=0.0)
    want = ref.cloud(frames, K_HAND, mode=0, **th0)
    got = ctx.map_cloud(fids, K_HAND, mode=0, imm_host_id=imm_ids, **th0)
    ref.assert_cloud_equal(got, want, "immature, minBS = 0")
    assert want["kept"][2, 0] == 70 and np.isnan(want["xyz"][want["first"][2]:want["first"][2] + 8]).all()
    assert (want["rgb"][want["first"][2]:want["first"][2] + 8 * 70] == (0, 255, 255)).all()
    # ---- all kept / none kept
    ref.assert_cloud_equal(ctx.map_cloud([10], K_HAND, mode=0, scaledTH=1e30, absTH=1.0, minBS=0.0), ref.cloud(frames[:1], K_HAND, mode=0, scaledTH=1e30, absTH=1.0, minBS=0.0), "all")
    none = ctx.map_cloud([10, 12], K_HAND, mode=0, scaledTH=1e30, absTH=1.0, minBS=2.0)
    assert none["n"] == 0 and none["first"].tolist() == [0, 0, 0] and (none["kept"] == 0).all() and (none["xyz"] == -77).all()
    # ---- an empty keyframe alone
    e = ctx.map_cloud([11], K_HAND, mode=0, **th)
    assert e["n"] == 0 and e["first"].tolist() == [0, 0]


def test_world_frame(gpu_ctx, hand_made):
    ctx = gpu_ctx
    lists, imm = hand_made
    fids = [13, 10, 12]
    frames = [dict(lists=lists[f]) for f in fids]
    rs = np.random.RandomState(21)
    T = np.zeros((3, 12), F)
    for k in range(3):
        q, _ = np.linalg.qr(rs.normal(0, 1, (3, 3)))
        T[k, :9] = q.reshape(-1); T[k, 9:] = rs.normal(0, 30, 3)
    th = dict(scaledTH=1e30, absTH=1.0, minBS=0.5)
    want = ref.cloud(frames, K_HAND, mode=1, camToWorld=T, **th)
    got = ctx.map_cloud(fids, K_HAND, mode=1, camToWorld=T, **th)
    ref.assert_cloud_equal(got, want, "world frame")
    cam = ref.cloud(frames, K_HAND, mode=1, **th)
    assert got["n"] == cam["first"][-1] > 1000 and (got["xyz"][:got["n"]].view(np.uint32) != cam["xyz"].view(np.uint32)).mean() > 0.9


# ------------------------------------------------------------------ contract
def test_cloud_is_repeatable_and_device_buffers_hold_it(gpu_ctx, hand_made):
    ctx = gpu_ctx
    lists, imm = hand_made
    kw = dict(mode=0, imm_host_id=[IMM_ID, -1, -1, -1], scaledTH=1e30, absTH=1.0, minBS=0.0)
    a = ctx.map_cloud([13, 10, 11, 12], K_HAND, **kw)
    b = ctx.map_cloud([13, 10, 11, 12], K_HAND, **kw)
    for k in ("xyz", "rgb", "first", "kept"):
        assert a[k].tobytes() == b[k].tobytes(), k
    xyz_dev, rgb_dev, n = ctx.map_cloud_dev()
    assert n == a["first"][-1] == a["n"] > 0
    assert ctx.read_device(xyz_dev, 12 * n).tobytes() == a["xyz"][:n].tobytes()
    assert ctx.read_device(rgb_dev, 3 * n).tobytes() == a["rgb"][:n].tobytes()


def test_update_changes_nothing_in_the_window(gpu_ctx, cases):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["C"]
    before, keep = _optimized(ctx, win, WU)
    th = fref.median_hessian(before)
    f0 = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    _flag_and_update(ctx, WU, win, before, frame_marg, last_gone)
    ctx.map_update(WU, None, np.nonzero(f0[0] != fref.KEEP)[0], np.where(f0[0][f0[0] != fref.KEEP] == fref.MARGINALIZE, 2, 3))
    wu.assert_same(before, wu.post_state(ctx, WU, win), what="post-state after sdso_map_update")
    f1 = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=th)
    for x, y in zip(f0, f1):
        assert x.tobytes() == y.tobytes()
    _release(ctx, WU)


def test_active_null_is_window_order(gpu_ctx, cases):
    ctx = gpu_ctx
    win, frame_marg, last_gone = cases["C"]
    post, keep = _optimized(ctx, win, WU)
    dec, _, _ = ctx.flag_points(WU, win["nf"], win["np"], frame_marg, last_gone, minIdepthH_marg=fref.median_hessian(post))
    gone = np.nonzero(dec != fref.KEEP)[0][::-1].astype(np.int32)
    w = dict(active=[[int(p) for p in np.nonzero((dec == fref.KEEP) & (win["host"] == h))[0]] for h in range(win["nf"])], gone=gone,
             gone_list=np.where(dec[gone] == fref.MARGINALIZE, 2, 3).astype(np.uint8))
    ctx.map_update(WU, None, w["gone"], w["gone_list"])
    _assert_lists(ctx, ref.lists_after(win, post, w), "active = NULL")
    _release(ctx, WU)


def test_update_refusals_leave_map_and_window_usable(gpu_ctx, cases):
    ctx, L = gpu_ctx, gpu_ctx.L
    win, frame_marg, last_gone = cases["C"]
    npts = win["np"]
    ctx.check(L.sdso_map_clear(ctx.h))
    wu.upload_pyramids(ctx, win)
    wu.upload(ctx, win, WU)
    assert ctx.map_update_raw(WU, None, [], []) == ERR_STATE and b"post-state" in _err(ctx)        # no optimize has ended
    wu.optimize(ctx, WU)
    post = wu.post_state(ctx, WU, win)
    dec, w, lists = _flag_and_update(ctx, WU, win, post, frame_marg, last_gone)
    _assert_lists(ctx, lists, "first good call")
    act = np.array([p for l in w["active"] for p in l], np.int32)
    g, gl = w["gone"], w["gone_list"]

    def bad(a, gone, glist, text, wid=WU):
        assert ctx.map_update_raw(wid, a, gone, glist) == ERR_ARG, text
        assert text in _err(ctx), (text, _err(ctx))

    x = act.copy(); x[0] = npts
    bad(x, g, gl, b"out of range")
    x = g.copy(); x[-1] = -1
    bad(act, x, gl, b"out of range")
    x = act.copy(); x[1] = x[0]
    bad(x, g, gl, b"twice")
    x = act.copy(); x[0] = g[0]
    bad(x, g, gl, b"twice")
    x = g.copy(); x[1] = x[0]
    bad(None, x, gl, b"twice")
    x = gl.copy(); x[0] = 1
    bad(act, g, x, b"gone_list")
    x = gl.copy(); x[-1] = 0
    bad(act, g, x, b"gone_list")
    bad(act[:-1], g, gl, b"n_active + n_gone")
    bad(act, g, gl, b"unknown window", wid=977)
    assert L.sdso_map_update(ctx.h, WU, None) == ERR_ARG
    _assert_lists(ctx, lists, "after the refusals")                               # the map is as it was (no list grew or was replaced)
    wu.assert_same(post, wu.post_state(ctx, WU, win), what="post-state after the refusals")
    # a good call afterwards still matches: the same update again appends the leaving points once more
    ctx.map_update(WU, act, g, gl)
    _assert_lists(ctx, ref.lists_after(win, post, w, before=lists), "good call after the refusals")
    # flagPointsForRemoval's marginalised points are linearised by sdso_ba_marginalize_points: the window no longer answers
    wu.marginalize_points(ctx, WU, win, (dec == fref.MARGINALIZE).astype(np.uint8))
    assert ctx.map_update_raw(WU, act, g, gl) == ERR_STATE and b"linearised" in _err(ctx)
    _release(ctx, WU)


def test_update_is_refused_inside_a_batch(gpu_ctx, cases):
    ctx, L = gpu_ctx, gpu_ctx.L
    win, frame_marg, last_gone = cases["C"]
    post, keep = _optimized(ctx, win, WU)
    dec, w, lists = _flag_and_update(ctx, WU, win, post, frame_marg, last_gone)
    ctx.check(L.sdso_ba_batch_create(ctx.h, 1, abi.ip(np.array([WU], np.int32))))
    act = np.array([p for l in w["active"] for p in l], np.int32)
    assert ctx.map_update_raw(WU, act, w["gone"], w["gone_list"]) == ERR_STATE and b"member of a batch" in _err(ctx)
    assert ctx.map_update_raw(WU, None, [], []) == ERR_STATE and b"member of a batch" in _err(ctx)
    _assert_lists(ctx, lists, "after the refusal inside a batch")
    _release(ctx, WU)                                                              # (releasing a member dissolves the batch)


def test_cloud_refusals_release_and_clear(gpu_ctx, hand_made):
    ctx, L = gpu_ctx, gpu_ctx.L
    lists, imm = hand_made
    th = dict(scaledTH=1e30, absTH=1.0, minBS=0.5)
    fids = [10, 12, 13]
    frames = [dict(lists=lists[f]) for f in fids]
    want = ref.cloud(frames, K_HAND, mode=1, **th)
    ref.assert_cloud_equal(ctx.map_cloud(fids, K_HAND, mode=1, **th), want, "first good call")

    def bad(ids, text, **kw):
        args = dict(th, mode=1, cap=8 * 2000)
        args.update(kw)
        rc, d = ctx.map_cloud_raw(ids, K_HAND, **args)
        assert rc == ERR_ARG and text in _err(ctx), (text, rc, _err(ctx))
        assert (d["xyz"] == -77).all() and (d["rgb"] == 77).all()

    bad([10, 99], b"unknown frameID")
    bad([10, 12], b"immature group", imm_host_id=[-1, IMM_ID + 1])
    bad([10, 12, 10], b"twice")
    bad([], b"n_frames")
    bad([10, 11, 12, 13, 20, 21, 22, 23, 24], b"n_frames")
    bad(fids, b"NaN", scaledTH=float("nan"))
    bad(fids, b"NaN", absTH=float("nan"))
    bad(fids, b"NaN", minBS=float("nan"))
    bound = 8 * sum(len(lists[f][l]) for f in fids for l in (1, 2, 3))
    assert bound > want["first"][-1]                                                # the refusal is decided on the bound, not on the outcome
    bad(fids, b"cap", cap=bound - 1)
    bad([12], b"cap", cap=8 * (64 + 65 + 70) - 1, imm_host_id=[IMM_ID])             # the immature group counts towards the bound
    assert L.sdso_map_cloud(ctx.h, None, None, None, None, None) == ERR_ARG
    assert L.sdso_map_get(ctx.h, 10, 4, None) == ERR_ARG and L.sdso_map_put(ctx.h, 10, 0, 0, None) == ERR_ARG
    ref.assert_cloud_equal(ctx.map_cloud(fids, K_HAND, mode=1, cap=bound, **th), want, "good call after the refusals")
    _assert_lists(ctx, lists, "after the refusals")
    # ---- release makes the id unknown; clear empties the map
    ctx.check(L.sdso_map_release_keyframe(ctx.h, 12))
    cnt = np.zeros(3, np.int32)
    assert L.sdso_map_counts(ctx.h, 12, abi.ip(cnt)) == ERR_ARG and b"unknown frameID" in _err(ctx)
    rc, _ = ctx.map_cloud_raw(fids, K_HAND, cap=bound, **th)
    assert rc == ERR_ARG and b"unknown frameID" in _err(ctx)
    ref.assert_cloud_equal(ctx.map_cloud([10, 13], K_HAND, mode=1, **th), ref.cloud([frames[0], frames[2]], K_HAND, mode=1, **th), "after the release")
    ctx.check(L.sdso_map_release_keyframe(ctx.h, 12))                               # releasing twice is not an error
    ctx.check(L.sdso_map_clear(ctx.h))
    for f in (10, 11, 13):
        assert L.sdso_map_counts(ctx.h, f, abi.ip(cnt)) == ERR_ARG
