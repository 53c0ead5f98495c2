"""sdso_ba_window_update_activated: the points an activation made enter the resident BA window device to device, and the window is the
one the all-host route makes — sdso_imm_activate_fetch, stage 7 built in NumPy by the rules of include/sdso_abi.h, sdso_ba_window_update.

Every comparison is np.array_equal (window_update_helpers.assert_same): every value is a copy or a fixed-order per-point expression, so
no tolerance appears.  The activation (tests/activate_cases.py) and the BA window (synth.ba_window) share the image size and nothing else:
the activated points land on the window's frames with the values the activation gave them.

What the CPU statement (activate_ref.activate, minObs = 1) gives on the four-frame case: toOptimize has 227 entries with statuses
-1 / 0 / 1 = 38 / 44 / 145; the 145 activated points sit on three hosts (115, 29, 1) and 6 / 13 / 126 of them have 1 / 2 / 3 IN residuals,
410 new residuals in all.  On full_window_cases.resident(): 1 206 entries, 761 activated on seven hosts, 666 of them with 7 IN residuals.
The preconditions below are asserted on the statement's records, so a changed fixture fails loudly."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import activate_cases as AC
import activate_ref as AR
import distmap_cases as DC
import full_window_cases as FW
import synth
import window_activated_helpers as wa
import window_update_helpers as wu

pytestmark = pytest.mark.gpu
W, H = wa.W, wa.H
SLOT = 2340                       # frames 0..3 of the activation window
SLOT_SEL, SLOT8 = 2350, 2360      # a full pyramid for sdso_pixel_select; frames 0..7 of the eight-keyframe activation
WN, WF, WS = 13, 14, 15           # window ids: path N, path F, the small window of the refusals
IDS_F, IDS_N = [2400, 2401, 2402, 2403], [2410, 2411, 2412, 2413]
BA_SEED = 4101


@pytest.fixture(scope="module")
def windows():
    """the 4-frame BA window with a history, and the frame that variant (a) appends: frame 4 of the 5-frame window of the same seed"""
    base = wu.with_history(synth.ba_window(w=W, h=H, nf=4, pts_per_kf=40, seed=BA_SEED), 31)
    b5 = synth.ba_window(w=W, h=H, nf=5, pts_per_kf=40, seed=BA_SEED)
    assert int(b5["frameID"][4]) not in [int(f) for f in base["frameID"]]
    new = {k: np.ascontiguousarray(b5[k][4:5]) for k in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID")}
    new["pyrs"] = [b5["pyrs"][4]]
    return base, new


@pytest.fixture(scope="module")
def env(gpu_ctx, oracle, windows):
    ctx = gpu_ctx
    base, new = windows
    c0 = AC.window(oracle)
    for f in range(4):
        ctx.upload_pyramid(SLOT + f, [c0["win"]["imgs"][f]])
    ctx.upload_pyramid(SLOT_SEL, synth.make_pyramid(np.ascontiguousarray(c0["win"]["imgs"][1][..., 0])))
    wu.upload_pyramids(ctx, base)
    ctx.upload_pyramid(wu.SLOT0 + int(new["frameID"][0]), new["pyrs"][0][:1])
    yield ctx
    wa.release_groups(ctx, IDS_F + IDS_N)
    for s in [SLOT + f for f in range(4)] + [SLOT_SEL]:
        ctx.L.sdso_release_pyramid(ctx.h, s)
    for w in (WN, WF, WS):
        ctx.L.sdso_ba_release_window(ctx.h, w)


def _case4(oracle):
    c = AC.window(oracle)
    return c, c["win"], [SLOT + f for f in range(4)]


def _case_sub(oracle):
    c = AC.window(oracle)
    return c, wa.sub_window(c["win"], [1, 3]), [SLOT + 1, SLOT + 3]


def _case_none(oracle):
    c = AC.window(oracle)
    w2 = wa.sub_window(c["win"], [0, 3])
    w2["flagged"][:] = 0
    w2["groups"] = [wa.keep_all(c["win"]["groups"][0]), None]
    return c, w2, [SLOT, SLOT + 3]


def _keyframe_edit(base, new):
    """the real keyframe edit: the newest frame is appended (stage 5) and the points of the two newest hosts observe it (stage 6)"""
    nf = base["nf"]
    add_res = [(int(p), nf) for p in np.nonzero(base["host"] >= nf - 2)[0]]
    payload = dict(add_frames=new, add_res_isNew=(np.random.RandomState(3).rand(len(add_res)) < 0.8).astype(np.uint8))
    return dict(n_add_frames=1, add_res=add_res), payload


def _upload_both(ctx, base):
    wu.upload(ctx, base, WN); wu.upload(ctx, base, WF)


def _preconditions(rec, hosts, residual_counts):
    """on the statement's records: all three statuses, at least `hosts` hosts, a point with every residual count named"""
    st = np.asarray(rec["status"])
    assert set(np.unique(st)) == {-1, 0, 1}
    act = st == 1
    assert len(np.unique(rec["frame"][act])) >= hosts
    n_in = (rec["res_state"][act] == wa.IN).sum(1)
    for k in residual_counts:
        assert (n_in == k).any(), k
    return int(act.sum()), int(n_in.sum())


def test_statement_preconditions(oracle):
    c, win, _ = _case4(oracle)
    rec = wa.statement(oracle, c, win, 1)
    assert len(rec["status"]) == 227 and _preconditions(rec, 3, (1, 2, 3)) == (145, 410)


@pytest.mark.parametrize("variant", ["identity_keyframe", "permuted", "outlier_stages", "sub_window", "nothing_activated"])
def test_path_n_equals_path_f(env, oracle, windows, variant):
    ctx = env
    base, new = windows
    _upload_both(ctx, base)
    maker, act_frame, edit, payload = _case4, [0, 1, 2, 3], {}, {}
    if variant == "identity_keyframe":          # (a) the activation's newest frame is the appended one
        act_frame = [0, 1, 2, 4]
        edit, payload = _keyframe_edit(base, new)
    elif variant == "permuted":                 # (b) a non-identity permutation onto the window's frames
        act_frame = [2, 0, 3, 1]
    elif variant == "outlier_stages":           # (c) stages 1-3 after an optimize, in the same call
        wu.optimize(ctx, WN); wu.optimize(ctx, WF)
        dN, dF = wu.post_state(ctx, WN, base), wu.post_state(ctx, WF, base)
        wu.assert_same(dN, dF, what="the two optimised windows")
        edit = wu.outlier_edit(base, dF)
        print("stage 1 drops", len(edit["drop_res"]), "stage 3 drops", int(edit["drop_point"].sum()))
        assert len(edit["drop_res"]) > 0
    elif variant == "sub_window":               # (d) nf_act = 2
        maker, act_frame = _case_sub, [3, 1]
    else:                                       # (e) nothing is selected: a plain update
        maker, act_frame = _case_none, [0, 3]
    c, win, _ = maker(oracle)
    want = wa.statement(oracle, c, win, 1)
    r = wa.run_pair(ctx, lambda: maker(oracle), base, WN, WF, act_frame, IDS_F[:len(act_frame)], IDS_N[:len(act_frame)], edit, payload, again=True)
    sN, _ = wa.assert_pair(ctx, r, WN, WF, variant)
    # the call's outputs against the statement's records
    _, _, idx = wa.stage7(want, act_frame)
    assert np.array_equal(r["act_index"], idx) and r["n_points"] == int((want["status"] == 1).sum())
    assert r["n_res"] == int((want["res_state"][want["status"] == 1] == wa.IN).sum())
    assert r["rc_again"] == wa.ERR_STATE                    # the result was consumed
    print(variant, "points", r["n_points"], "residuals", r["n_res"], "window", r["sizes"])
    if variant == "nothing_activated":
        assert r["n_points"] == 0 and r["n_res"] == 0 and r["sizes"] == dict(nf=base["nf"], np=base["np"], nr=base["nr"])
    elif variant == "sub_window":
        assert 0 < r["n_points"] < 145
    else:
        assert r["n_points"] == 145 and r["n_res"] == 410
    # the appended points carry the records' values, on the hosts the map names (window order groups the points by host)
    ps = np.array(r["maps"][1])
    k = -1 - ps[ps < 0]
    assert np.array_equal(sN["idepth"][ps < 0], want["idepth"][idx][k], equal_nan=True)
    hosts_new = np.array([act_frame[int(f)] for f in want["frame"][idx]], np.int64)[k]
    assert (np.diff(hosts_new) >= 0).all()
    if variant == "permuted":
        frames = set(int(f) for f in want["frame"][idx])
        assert set(hosts_new.tolist()) == {act_frame[f] for f in frames} != frames and len(frames) >= 3


def test_optimize_after_the_edit(env, oracle, windows):
    ctx = env
    base, new = windows
    _upload_both(ctx, base)
    edit, payload = _keyframe_edit(base, new)
    r = wa.run_pair(ctx, lambda: _case4(oracle), base, WN, WF, [0, 1, 2, 4], IDS_F, IDS_N, edit, payload)
    assert r["rcF"] == 0 and r["rcN"] == 0, r["errN"]
    s = r["sizes"]
    wu.optimize(ctx, WF, 3)
    pF = wu.post_state(ctx, WF, s)
    new_res = np.array(r["maps"][2]) <= -1 - len(edit["add_res"])          # stage 7's residuals follow stage 6's
    assert new_res.sum() == 410
    assert (pF["state_state"][new_res] == wa.IN).any()                      # the optimize read the new rows
    wu.optimize(ctx, WN, 3)
    wu.assert_same(wu.post_state(ctx, WN, s), pF, what="optimize after the edit")


def _scratch_users(ctx, c):
    """calls that use the ctx scratch, each with more bytes than the activation's records reach"""
    rs = np.random.RandomState(5)
    n = 6000
    DC.dm_make(ctx, W, H, c["win"]["KRKi"], c["win"]["Kt"], rs.randint(0, 3, n), rs.uniform(3, W - 4, n), rs.uniform(3, H - 4, n), rs.uniform(0.01, 0.2, n))
    pot, num = C.c_int(3), C.c_int(0)
    m = np.zeros((H, W), np.float32)
    ctx.check(ctx.L.sdso_pixel_select(ctx.h, SLOT_SEL, 1500.0, 1, 1.0, C.byref(pot), abi.fp(m), C.byref(num)))
    n = 2000                                                                # more points than the activation had candidates (1 297)
    P, d = abi.make_trace_points(n, rs.uniform(20, W - 20, n), rs.uniform(20, H - 20, n), np.ones((n, 8)), np.ones((n, 8)), np.ones((n, 4)), np.ones(n))
    st = np.zeros(n, np.uint8)
    K4 = np.ascontiguousarray(c["win"]["K4"], np.float32)
    ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, SLOT + 3, abi.fp(K4), 0.5, 1, C.byref(P), abi.bp(st)))


def test_records_survive_other_calls(env, oracle, windows):
    ctx = env
    base, _ = windows
    _upload_both(ctx, base)
    c0 = AC.window(oracle)
    assert sum(len(S["u"]) for S in c0["win"]["groups"][:3]) < 2000
    r = wa.run_pair(ctx, lambda: _case4(oracle), base, WN, WF, [0, 1, 2, 3], IDS_F, IDS_N, between=lambda: _scratch_users(ctx, c0))
    wa.assert_pair(ctx, r, WN, WF, "records after other users of the scratch")
    assert r["n_points"] == 145


def _light(ctx, wid, s):
    """what the getters that change nothing give: sdso_ba_get_state and, where the window has one, its order"""
    st, idp, rs_ = np.zeros((s["nf"], 10)), np.zeros(s["np"], np.float32), np.zeros(s["nr"], np.uint8)
    ctx.check(ctx.L.sdso_ba_get_state(ctx.h, wid, abi.dp(st), abi.fp(idp), abi.bp(rs_)))
    return dict(state=st, idepth=idp, res_state=rs_, order=np.concatenate(wu.get_order(ctx, wid, s["nf"], s["np"], s["nr"])))


def test_refusals_leave_everything_alone(env, oracle, windows):
    ctx, L = env, env.L
    base, new = windows
    empty, keep_empty = wa.edit_abi({})

    def refused(E, af, wid=WN):
        rc = ctx.window_update_activated(wid, E, af, 256)[0]
        return rc, L.sdso_last_error(ctx.h)

    # ---- before any activation on the ctx: a fresh one with a window of its own
    small = dict(synth.ba_window(w=320, h=240, nf=4, pts_per_kf=20, seed=4107))
    small["frameID"] = np.arange(20, 24, dtype=np.int32)
    fresh = abi.Context(0)
    try:
        wu.upload_pyramids(fresh, small)
        wu.upload(fresh, small, WS)
        assert fresh.window_update_activated(WS, empty, [0, 1, 2, 3], 256)[0] == wa.ERR_STATE
        assert b"sdso_imm_activate" in fresh.L.sdso_last_error(fresh.h)
        wu.upload(fresh, small, WF)                                        # WF never takes a call
        wu.assert_same(wu.snapshot(fresh, WS, small), wu.snapshot(fresh, WF, small), what="refused before any activation")
    finally:
        fresh.close()
    # ---- WN takes every refused call, WF none: two uploads of the same window and one empty update each, so that both have an order to show
    _upload_both(ctx, base)
    assert wu.update(ctx, WN, {}) == 0 and wu.update(ctx, WF, {}) == 0
    wu.upload_pyramids(ctx, small)
    wu.upload(ctx, small, WS)
    # ---- an activation whose result stays unconsumed through every refusal
    c, win, slots = _case4(oracle)
    wa.activate_on_device(ctx, c, win, IDS_N, slots, 1, False)
    groups = wa.get_groups(ctx, IDS_N)
    e7, p7, _ = wa.stage7(wa.statement(oracle, *_case4(oracle)[:2], 1), [0, 1, 2, 3])
    E7, keep7 = wa.edit_abi(e7, p7)
    Egone, keep_gone = wa.edit_abi(dict(drop_point=(base["host"] == 0).astype(np.uint8), remove_frames=[0]))
    got = dict(stage7=refused(E7, [0, 1, 2, 3]), null_map=refused(empty, None), out_of_range=refused(empty, [0, 1, 2, 4]), negative=refused(empty, [0, -1, 2, 3]),
               duplicate=refused(empty, [0, 1, 1, 3]), leaving=refused(Egone, [0, 1, 2, 3]), small_window=refused(empty, [0, 1, 2, 3], WS),
               unknown_window=refused(empty, [0, 1, 2, 3], 999))
    want = dict(stage7=(wa.ERR_ARG, b"stage 7 of the edit must be empty"), null_map=(wa.ERR_ARG, b"null act_frame"), out_of_range=(wa.ERR_ARG, b"out of range of the edited window"),
                negative=(wa.ERR_ARG, b"out of range of the edited window"), duplicate=(wa.ERR_ARG, b"two activation frames mapped to one window frame"),
                leaving=(wa.ERR_ARG, b"leaves in stage 4"), small_window=(wa.ERR_ARG, b"w / h differ"), unknown_window=(wa.ERR_ARG, b""))
    for k in want:                                                         # the stated code, from the rule that the case is about
        assert got[k][0] == want[k][0] and want[k][1] in got[k][1], (k, got[k])
    sb = dict(nf=base["nf"], np=base["np"], nr=base["nr"])
    wu.assert_same(_light(ctx, WN, sb), _light(ctx, WF, sb), what="after the refusals outside a batch")
    small_took_a_call = wu.snapshot(ctx, WS, small)
    # ---- inside a batch: the getters a member allows, then the batch moves on to WS (sdso_ba_batch_create dissolves the one before) and
    # WN, still the window that took all nine calls, shows everything
    ids = np.array([WN], np.int32)
    ctx.check(L.sdso_ba_batch_create(ctx.h, 1, abi.ip(ids)))
    rc, why = refused(empty, [0, 1, 2, 3])
    assert rc == wa.ERR_STATE and b"member of a batch" in why, (rc, why)
    wu.assert_same(_light(ctx, WN, sb), _light(ctx, WF, sb), what="after the refusal inside the batch")
    ids = np.array([WS], np.int32)
    ctx.check(L.sdso_ba_batch_create(ctx.h, 1, abi.ip(ids)))
    wu.upload(ctx, small, WS)                                              # (dissolves that one in turn; WS is fresh now)
    wu.assert_same(wu.snapshot(ctx, WN, sb), wu.snapshot(ctx, WF, sb), what="the window of the nine refused calls")
    wu.assert_same(small_took_a_call, wu.snapshot(ctx, WS, small), what="the 320 x 240 window")
    wa.same_groups(wa.get_groups(ctx, IDS_N), groups)
    # ---- the records are still there and unconsumed: on two fresh uploads the call now succeeds and equals path F
    _upload_both(ctx, base)
    rec = ctx.imm_activate_fetch(sum(len(S["u"]) for S in AC.window(oracle)["win"]["groups"][:3]), 227, 4)
    e7, p7, idx = wa.stage7(rec, [0, 1, 2, 3])
    assert wu.update(ctx, WF, e7, p7) == 0
    rc, n_pt, n_res, act_index = ctx.window_update_activated(WN, empty, [0, 1, 2, 3], 227)
    assert rc == 0 and n_pt == 145 and n_res == 410 and np.array_equal(act_index, idx)
    s, _ = wa.sizes_after(base, e7)
    wu.assert_same(wu.snapshot(ctx, WN, s), wu.snapshot(ctx, WF, s), what="after the refused calls")
    wa.release_groups(ctx, IDS_N)


def test_eight_keyframes(gpu_ctx, oracle):
    """One case at the full window: full_window_cases.resident() into a synth.ba_window of eight frames, identity map."""
    ctx = gpu_ctx
    base = wu.with_history(synth.ba_window(w=W, h=H, nf=8, pts_per_kf=40, seed=4103), 37)
    c, cs = FW.resident(), FW.resident()
    want = AR.activate(oracle, cs["win"], FW.ref_map(cs), 1, cs["min_act_dist"])["records"]
    act = want["status"] == 1
    assert len(np.unique(want["frame"][act])) >= 4 and ((want["res_state"][act] == wa.IN).sum(1) == 7).any()
    ids_f, ids_n = list(range(2420, 2428)), list(range(2430, 2438))
    slots = [SLOT8 + f for f in range(8)]

    def maker():
        k = FW.resident()
        return k, k["win"], slots

    try:
        for f in range(8):
            ctx.upload_pyramid(slots[f], [c["win"]["imgs"][f]])
        wu.upload_pyramids(ctx, base)
        wu.upload(ctx, base, WN); wu.upload(ctx, base, WF)
        r = wa.run_pair(ctx, maker, base, WN, WF, list(range(8)), ids_f, ids_n)
        wa.assert_pair(ctx, r, WN, WF, "eight keyframes")
        _, _, idx = wa.stage7(want, list(range(8)))
        assert np.array_equal(r["act_index"], idx) and r["n_points"] == int(act.sum()) > 700
        print("eight keyframes: points", r["n_points"], "residuals", r["n_res"], "window", r["sizes"])
    finally:
        wa.release_groups(ctx, ids_f + ids_n)
        for s in slots:
            ctx.L.sdso_release_pyramid(ctx.h, s)
        for w in (WN, WF):
            ctx.L.sdso_ba_release_window(ctx.h, w)
