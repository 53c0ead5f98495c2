"""What the sdso_ba_window_update_activated / sdso_distmap_make_from_window tests share: stage 7 of an edit from the records of an
activation by the rules of include/sdso_abi.h (the tail of optimizeImmaturePoint, FullSystemOptPoint.cpp:196-237, and STEP 4 of
activatePointsMT, FullSystem.cpp:919-945), and the two paths to the edited window.
  path N: sdso_imm_activate, then sdso_ba_window_update_activated (the records never leave the device);
  path F: sdso_imm_activate + sdso_imm_activate_fetch, stage 7 built here in NumPy, sdso_ba_window_update.
Both run on two uploads of the same window, from two puts of the same groups."""
import copy
import ctypes as C

import numpy as np

from sdso_amd import abi
import activate_cases as AC
import activate_ref as AR
import distmap_cases as DC
import immature_cases as Cs
import immature_ref as R
import window_edit_cases as cases
import window_edit_ref as ref
import window_update_helpers as wu

W, H = Cs.W, Cs.H
IN = 0                            # ResState::IN (Residuals.h:49)
ERR_ARG, ERR_STATE = -1, -4


# ---- the resident groups of an activation (what the sdso_imm_activate tests do, as plain functions: tools/ uses them too)
def put_groups(ctx, ids, groups):
    for hid, S in zip(ids, groups):
        if S is not None:
            ctx.imm_put(hid, S, W, H)


def release_groups(ctx, ids):
    for hid in ids:
        ctx.L.sdso_imm_release_host(ctx.h, hid)


def get_groups(ctx, ids):
    """sdso_imm_get of every id; None where the ctx holds no such group"""
    return [ctx.imm_get(i) if ctx.L.sdso_imm_get(ctx.h, i, C.byref(abi.TracePoints()), None) == 0 else None for i in ids]


def same_groups(got, want):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), j
        if a is not None:
            assert R.same(a, b) is None, "frame %d: %s differs" % (j, R.same(a, b))


def make_map(ctx, c):
    """sdso_distmap_make from the case's seeds"""
    pg, u, v, idp = c["seeds"]
    DC.dm_make(ctx, W, H, c["win"]["KRKi"], c["win"]["Kt"], pg, u, v, idp)


def activate_args(win, ids, slots):
    """the keyword arguments of Context.imm_activate / imm_activate_raw for a window of activate_cases"""
    return dict(host_id=ids, frame_slot=slots, host_flagged=win["flagged"], KRKi=win["KRKi"], Kt=win["Kt"], pair_R=win["pair_R"], pair_t=win["pair_t"],
                pair_aff=win["pair_aff"], w=W, h=H, K4=win["K4"])


def sub_window(win, frames):
    """the window restricted to `frames` (the last one is the newest)"""
    nf0 = len(win["groups"])
    pick = [a * nf0 + b for a in frames for b in frames]
    return dict(groups=[win["groups"][f] for f in frames[:-1]] + [None], imgs=[win["imgs"][f] for f in frames], flagged=win["flagged"][frames].copy(),
                KRKi=win["KRKi"][frames[:-1]].copy(), Kt=win["Kt"][frames[:-1]].copy(), pair_R=win["pair_R"][pick].copy(), pair_t=win["pair_t"][pick].copy(),
                pair_aff=win["pair_aff"][pick].copy(), K4=win["K4"], w=W, h=H)


def keep_all(S):
    """a group none of whose entries STEP 2 deletes or selects: finite intervals, IPS_UNINITIALIZED (not activatable, the host not flagged)"""
    S = copy.deepcopy(S)
    S["idepth_max"][~np.isfinite(S["idepth_max"])] = np.float32(1)
    S["lastTraceStatus"][:] = R.UNINITIALIZED
    return S


def stage7(rec, act_frame):
    """records of an activation (dict of arrays in toOptimize order) -> (edit part, payload part, act_index)"""
    idx = np.nonzero(np.asarray(rec["status"]) == 1)[0]
    rs = np.asarray(rec["res_state"])
    nf_act = rs.shape[1]
    hosts = [int(act_frame[int(rec["frame"][p])]) for p in idx]
    pt_res = [(q, int(act_frame[f])) for q, p in enumerate(idx) for f in range(nf_act) if rs[p, f] == IN]
    pts = dict(u=rec["u"][idx], v=rec["v"][idx], idepth=rec["idepth"][idx], idepth_zero=rec["idepth"][idx], color=rec["color"][idx], weights=rec["weights"][idx],
               hasDepthPrior=np.zeros(len(idx), np.uint8))
    return dict(add_points=hosts, pt_res=pt_res), dict(add_points=pts, pt_res_state=np.full(len(pt_res), IN, np.uint8)), idx.astype(np.int32)


def edit_abi(edit, payload=None):
    """the BAWindowEdit of wu.update, for the calls that take it directly"""
    pl = dict(payload or {})
    if "add_frames" in pl:
        af = dict(pl["add_frames"])
        af["frame_slot"] = [wu.SLOT0 + int(f) for f in af["frameID"]]
        pl["add_frames"] = af
    return cases.to_abi(edit, pl)


def sizes_after(win, edit):
    """-> (dict(nf, np, nr) of the edited window, its maps as sdso_ba_window_get_order returns them)"""
    maps = ref.apply_edit(win["nf"], win["host"], win["res_point"], win["res_target"], edit)
    return dict(nf=len(maps[0]), np=len(maps[1]), nr=len(maps[2])), tuple(list(int(x) for x in m) for m in maps)


def activate_on_device(ctx, c, win, ids, slots, min_obs, fetch):
    """put the groups, make the map from the case's seeds, sdso_imm_activate [+ fetch] -> (counts, records or None)"""
    put_groups(ctx, ids, win["groups"])
    make_map(ctx, c)
    args = activate_args(win, ids, slots)
    if fetch:
        return ctx.imm_activate(min_obs=min_obs, min_act_dist=float(c["min_act_dist"]), **args)
    rc, counts = ctx.imm_activate_raw(min_obs=min_obs, min_act_dist=float(c["min_act_dist"]), **args)
    ctx.check(rc)
    return counts, None


def statement(oracle, c, win, min_obs):
    """activate_ref.activate on a fresh copy of the case -> its records"""
    _, m = AC.ref_map(c)
    return AR.activate(oracle, win, m, min_obs, c["min_act_dist"])["records"]


def run_pair(ctx, case_maker, base, wn, wf, act_frame, ids_f, ids_n, edit=None, payload=None, min_obs=1, between=None, again=False):
    """Both paths from the windows wn / wf as they stand (two uploads of `base`, or two equal histories).  case_maker() -> a fresh
    (c, win, slots).  -> dict(rcF, rcN, n_points, n_res, act_index, rec (path F's fetch), edit (with stage 7), sizes, maps, rc_again)"""
    edit, payload = dict(edit or {}), dict(payload or {})
    out = {}
    c, win, slots = case_maker()
    counts, rec = activate_on_device(ctx, c, win, ids_f, slots, min_obs, True)
    e7, p7, idx = stage7(rec, act_frame)
    full_edit, full_payload = dict(edit, **e7), dict(payload, **p7)
    out["rcF"] = wu.update(ctx, wf, full_edit, full_payload)
    release_groups(ctx, ids_f)
    c, win, slots = case_maker()
    counts_n, _ = activate_on_device(ctx, c, win, ids_n, slots, min_obs, False)
    if between is not None:
        between()
    E, keep = edit_abi(edit, payload)
    out["rcN"], out["n_points"], out["n_res"], out["act_index"] = ctx.window_update_activated(wn, E, act_frame, int(counts_n[4]))
    out["errN"] = ctx.L.sdso_last_error(ctx.h)
    if again:
        E0, keep0 = edit_abi({})
        out["rc_again"] = ctx.window_update_activated(wn, E0, act_frame, int(counts_n[4]))[0]
    release_groups(ctx, ids_n)
    out.update(rec=rec, counts=counts, counts_n=counts_n, want_index=idx, edit=full_edit, n_pt_res=len(e7["pt_res"]))
    out["sizes"], out["maps"] = sizes_after(base, full_edit)
    return out


def assert_pair(ctx, r, wn, wf, what):
    """path N == path F: the call's outputs, the order, and every array of wu.snapshot"""
    assert r["rcF"] == 0 and r["rcN"] == 0, (what, r["rcF"], r["rcN"], r["errN"])
    assert np.array_equal(r["counts"], r["counts_n"]), what
    assert r["n_points"] == len(r["want_index"]) and r["n_res"] == r["n_pt_res"], (what, r["n_points"], r["n_res"])
    assert np.array_equal(r["act_index"], r["want_index"]), what
    s = r["sizes"]
    oN, oF = wu.get_order(ctx, wn, s["nf"], s["np"], s["nr"]), wu.get_order(ctx, wf, s["nf"], s["np"], s["nr"])
    assert oN == oF == r["maps"], what
    sN, sF = wu.snapshot(ctx, wn, s), wu.snapshot(ctx, wf, s)
    wu.assert_same(sN, sF, what=what)
    return sN, sF
