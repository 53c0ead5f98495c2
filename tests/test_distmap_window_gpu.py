"""sdso_distmap_make_from_window: makeDistanceMap (CoarseTracker.cpp:1216-1255) + growDistBFS on the points of a resident BA window equals
sdso_distmap_make fed from sdso_ba_get_state and the window's u, v, host — byte for byte, at three moments of the window's life; and the
chain make_from_window -> sdso_imm_activate -> sdso_ba_window_update_activated equals the all-host route end to end.

The geometries are those of the window's four frames into a fifth pose, one of them pushed sideways so that a part of its points leaves
the level-1 image (any float values do for a parity test; 0 < n_seeds < np is asserted on the host route's result)."""
import numpy as np
import pytest

from sdso_amd import abi
import activate_cases as AC
import distmap_cases as DC
import synth
import window_activated_helpers as wa
import window_update_helpers as wu

pytestmark = pytest.mark.gpu
W, H = wa.W, wa.H
SLOT = 2370                       # frames 0..3 of the activation window
WN, WF, WS = 16, 17, 18
IDS_F, IDS_N = [2440, 2441, 2442, 2443], [2450, 2451, 2452, 2453]
f32 = np.float32


@pytest.fixture(scope="module")
def problem():
    base = wu.with_history(synth.ba_window(w=W, h=H, nf=4, pts_per_kf=40, seed=4101), 31)
    b5 = synth.ba_window(w=W, h=H, nf=5, pts_per_kf=40, seed=4101)
    KRKi, Kt = DC.window_geoms(np.concatenate([base["evalPT"], b5["evalPT"][4:5]]), tuple(float(x) for x in base["calib_value_scaled"]))
    fxs = synth.level_intrinsics(*[float(x) for x in base["calib_value_scaled"]], 2)[0]
    Kt[1] = np.array([6.0 * fxs[1], 0, 0], f32)                 # frame 1 sideways: its nearer points leave the map
    return base, KRKi, Kt


@pytest.fixture(scope="module")
def env(gpu_ctx, problem):
    ctx = gpu_ctx
    wu.upload_pyramids(ctx, problem[0])
    yield ctx
    for w in (WN, WF, WS):
        ctx.L.sdso_ba_release_window(ctx.h, w)


def _host_route(ctx, wid, win, KRKi, Kt, frames=None):
    """sdso_ba_get_state + the window's u, v, host -> sdso_distmap_make; frames: the hosts whose points take part (default all)"""
    idp = np.zeros(win["np"], f32)
    ctx.check(ctx.L.sdso_ba_get_state(ctx.h, wid, None, abi.fp(idp), None))
    keep = np.ones(win["np"], bool) if frames is None else np.isin(win["host"], frames)
    n = DC.dm_make(ctx, W, H, KRKi, Kt, win["host"][keep], win["u"][keep], win["v"][keep], idp[keep])
    return n, DC.dm_get(ctx, W, H), idp


def _both(ctx, wid, win, KRKi, Kt, what):
    n_h, m_h, idp = _host_route(ctx, wid, win, KRKi, Kt)
    rc, n_w = ctx.distmap_make_from_window(wid, W, H, KRKi, Kt)
    assert rc == 0, ctx.L.sdso_last_error(ctx.h)
    m_w = DC.dm_get(ctx, W, H)
    print(what, "seeds", n_h, "of", win["np"])
    assert 0 < n_h < win["np"], what
    assert n_w == n_h and np.array_equal(m_w, m_h), what
    return idp, m_h


def test_equals_the_host_route_through_the_windows_life(env, problem):
    ctx = env
    base, KRKi, Kt = problem
    wu.upload(ctx, base, WN)
    idp0, m0 = _both(ctx, WN, base, KRKi, Kt, "after the upload")
    assert np.array_equal(idp0, base["idepth"])
    # ---- an optimize moves the idepths
    wu.optimize(ctx, WN)
    d = wu.post_state(ctx, WN, base)
    idp1, m1 = _both(ctx, WN, base, KRKi, Kt, "after an optimize")
    assert (idp1 != idp0).sum() > base["np"] // 2
    # ---- an update removes points and reorders the rest
    edit = wu.outlier_edit(base, d)
    drop = edit["drop_point"].copy()
    drop[::5] = 1
    edit["drop_point"] = drop
    edit["remove_points"] = [int(p) for p in np.nonzero(drop == 0)[0][3::17]]
    w2, maps = wu.flatten(base, wu.values_from_post(base, d), edit, {})
    assert wu.update(ctx, WN, edit) == 0, ctx.L.sdso_last_error(ctx.h)
    assert w2["np"] < base["np"] and list(maps[1]) != sorted(maps[1])
    _both(ctx, WN, w2, KRKi, Kt, "after an update")


def test_skip_no_synchronisation_and_refusals(env, problem):
    ctx = env
    base, KRKi, Kt = problem
    wu.upload(ctx, base, WN)
    # ---- skip on the last frame: the host route without that frame's points
    n_h, m_h, _ = _host_route(ctx, WN, base, KRKi, Kt, frames=[0, 1, 2])
    rc, n_w = ctx.distmap_make_from_window(WN, W, H, KRKi, Kt, skip=[0, 0, 0, 1])
    assert rc == 0 and n_w == n_h and np.array_equal(DC.dm_get(ctx, W, H), m_h)
    n_all, m_all, _ = _host_route(ctx, WN, base, KRKi, Kt)
    assert n_all > n_h and not np.array_equal(m_all, m_h)
    # ---- n_seeds = NULL: no synchronisation inside the call; the map is the same
    DC.dm_make(ctx, W, H, KRKi, Kt, np.zeros(1, np.int32), np.array([5.0], f32), np.array([5.0], f32), np.array([0.1], f32))     # (another map in between)
    rc, n_w = ctx.distmap_make_from_window(WN, W, H, KRKi, Kt, count=False)
    assert rc == 0 and n_w is None and np.array_equal(DC.dm_get(ctx, W, H), m_all)
    # ---- refusals: the previous map stays valid and unchanged
    small = dict(synth.ba_window(w=320, h=240, nf=4, pts_per_kf=20, seed=4107))
    small["frameID"] = np.arange(20, 24, dtype=np.int32)
    wu.upload_pyramids(ctx, small)
    wu.upload(ctx, small, WS)
    got = dict(unknown=ctx.distmap_make_from_window(999, W, H, KRKi, Kt)[0], wrong_wh=ctx.distmap_make_from_window(WN, 320, 240, KRKi, Kt)[0],
               wrong_wh_small=ctx.distmap_make_from_window(WS, W, H, KRKi, Kt)[0], null_geom=ctx.distmap_make_from_window(WN, W, H, None, None)[0])
    assert got == dict(unknown=wa.ERR_ARG, wrong_wh=wa.ERR_ARG, wrong_wh_small=wa.ERR_ARG, null_geom=wa.ERR_ARG), got
    assert np.array_equal(DC.dm_get(ctx, W, H), m_all)


def test_chain_equals_the_all_host_route(env, oracle, problem):
    """make_from_window -> sdso_imm_activate -> sdso_ba_window_update_activated against sdso_ba_get_state + sdso_distmap_make ->
    sdso_imm_activate + fetch -> sdso_ba_window_update, at the four-frame activation: the window's points are the seeds of the map the
    activation selects against, with the activation's own geometries."""
    ctx = env
    base, _, _ = problem
    c0 = AC.window(oracle)
    for f in range(4):
        ctx.upload_pyramid(SLOT + f, [c0["win"]["imgs"][f]])
    slots = [SLOT + f for f in range(4)]
    act_frame = [0, 1, 2, 3]
    KRKi4 = np.concatenate([c0["win"]["KRKi"], c0["win"]["KRKi"][:1]])      # a geometry for every window frame; the newest is skipped
    Kt4 = np.concatenate([c0["win"]["Kt"], c0["win"]["Kt"][:1]])
    skip = [0, 0, 0, 1]
    try:
        wu.upload(ctx, base, WN); wu.upload(ctx, base, WF)
        # ---- route F
        c = AC.window(oracle)
        wa.put_groups(ctx, IDS_F, c["win"]["groups"])
        n_f, m_f, _ = _host_route(ctx, WF, base, KRKi4, Kt4, frames=[0, 1, 2])
        counts_f, rec = ctx.imm_activate(min_obs=1, min_act_dist=float(c["min_act_dist"]), **wa.activate_args(c["win"], IDS_F, slots))
        e7, p7, idx = wa.stage7(rec, act_frame)
        assert wu.update(ctx, WF, e7, p7) == 0, ctx.L.sdso_last_error(ctx.h)
        map_f = DC.dm_get(ctx, W, H)
        wa.release_groups(ctx, IDS_F)
        # ---- route N
        c = AC.window(oracle)
        wa.put_groups(ctx, IDS_N, c["win"]["groups"])
        rc, _ = ctx.distmap_make_from_window(WN, W, H, KRKi4, Kt4, skip=skip, count=False)
        assert rc == 0, ctx.L.sdso_last_error(ctx.h)
        rc, counts_n = ctx.imm_activate_raw(min_obs=1, min_act_dist=float(c["min_act_dist"]), **wa.activate_args(c["win"], IDS_N, slots))
        assert rc == 0, ctx.L.sdso_last_error(ctx.h)
        E0, keep0 = wa.edit_abi({})
        rc, n_pt, n_res, act_index = ctx.window_update_activated(WN, E0, act_frame, int(counts_n[4]))
        assert rc == 0, ctx.L.sdso_last_error(ctx.h)
        map_n = DC.dm_get(ctx, W, H)
        wa.release_groups(ctx, IDS_N)
        print("chain: seeds", n_f, "counts", list(counts_n[:9]), "points", n_pt, "residuals", n_res)
        assert 0 < n_f and np.array_equal(counts_n, counts_f) and counts_n[7] > 20
        assert n_pt == len(idx) and np.array_equal(act_index, idx) and n_res == len(e7["pt_res"])
        assert np.array_equal(map_n, map_f)
        s, maps = wa.sizes_after(base, e7)
        assert wu.get_order(ctx, WN, s["nf"], s["np"], s["nr"]) == wu.get_order(ctx, WF, s["nf"], s["np"], s["nr"]) == maps
        wu.assert_same(wu.snapshot(ctx, WN, s), wu.snapshot(ctx, WF, s), what="the chain")
    finally:
        wa.release_groups(ctx, IDS_F + IDS_N)
        for s_ in slots:
            ctx.L.sdso_release_pyramid(ctx.h, s_)
