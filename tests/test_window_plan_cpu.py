"""sdso_ba_window_plan (the host half of sdso_ba_window_update, no ctx) against the Python statement of the seven stages
(tests/window_edit_ref.py, pinned by tests/test_window_edit_ref.py) on seeded random edits of synth.ba_window windows, and every edit
the reference could not perform refused with SDSO_ERR_ARG."""
import numpy as np
import pytest

import synth
import window_edit_cases as cases
import window_edit_ref as ref

SDSO_ERR_ARG = -1


@pytest.fixture(scope="module")
def windows():
    return {nf: synth.ba_window(w=320, h=240, nf=nf, pts_per_kf=40, seed=3100 + nf) for nf in (3, 5, 8)}


def _ints(win):
    return win["nf"], win["host"], win["res_point"], win["res_target"]


def _specs():
    """(name, nf, random_edit arguments)"""
    out = []
    for nf in (3, 5, 8):
        out.append(("drops_%d" % nf, nf, dict()))
        out.append(("shuffled_%d" % nf, nf, dict(shuffle_drops=True, res_frac=0.3)))
        out.append(("empty_host_%d" % nf, nf, dict(empty_host=1)))
        out.append(("keyframe_%d" % nf, nf, dict(remove_frames=[0], n_add_frames=1, n_add_points=25)))
    out.append(("two_frames_leave_8", 8, dict(remove_frames=[2, 0], n_add_frames=2, n_add_points=30)))
    out.append(("grow_5", 5, dict(n_add_frames=3, n_add_points=40, add_res_frac=0.8)))
    return out


def test_plan_matches_the_model_on_random_edits(windows):
    res_total = res_gone = pts_total = pts_gone = unsorted_lists = hosts_differ = 0
    for k, (name, nf, kw) in enumerate(_specs()):
        win = windows[nf]
        nf, host, rp, rt = _ints(win)
        edit = cases.random_edit(np.random.RandomState(700 + k), nf, host, rp, rt, **kw)
        want = ref.apply_edit(nf, host, rp, rt, edit)
        rc, fs, ps, rs_ = cases.c_plan(nf, host, rp, rt, edit)
        assert rc == 0, name
        assert (fs, ps, rs_) == tuple(list(x) for x in want), name
        # ---- what the cases exercise
        res_total += len(rp); res_gone += len(rp) - sum(1 for r in want[2] if r >= 0)
        pts_total += len(host); pts_gone += len(host) - sum(1 for p in want[1] if p >= 0)
        h2, rp2, rt2 = ref.flatten(nf, host, rp, rt, edit, want)
        for p in range(len(h2)):
            t = rt2[rp2 == p]
            unsorted_lists += bool(np.any(np.diff(t) < 0))
        for f in range(nf):
            lst = [p for p in range(len(host)) if host[p] == f]
            flagged = [p for p in lst if edit["drop_point"][p]]
            hosts_differ += ref.remove_points_in_order(lst, flagged) != ref.drop_points_rescan(lst, flagged)
        if "empty_host" in kw:
            assert not any(p >= 0 and host[p] == 1 for p in want[1]) and 1 in want[0], name      # the host stays, its list is empty
    assert res_gone >= 0.1 * res_total and pts_gone >= 0.1 * pts_total
    assert unsorted_lists > 0 and hosts_differ > 0


def test_empty_edit_is_the_identity(windows):
    for nf, win in windows.items():
        nf, host, rp, rt = _ints(win)
        rc, fs, ps, rs_ = cases.c_plan(nf, host, rp, rt, {})
        assert rc == 0 and fs == list(range(nf)) and ps == list(range(len(host))) and rs_ == list(range(len(rp)))


def test_every_point_leaves(windows):
    win = windows[5]
    nf, host, rp, rt = _ints(win)
    npts = len(host)
    half = [int(p) for p in np.random.RandomState(5).permutation(npts)[:npts // 2]]
    flags = np.ones(npts, np.uint8); flags[half] = 0
    edit = dict(remove_points=half, drop_point=flags)
    rc, fs, ps, rs_ = cases.c_plan(nf, host, rp, rt, edit)
    assert rc == 0 and fs == list(range(nf)) and ps == [] and rs_ == []
    assert ref.apply_edit(nf, host, rp, rt, edit) == (list(range(nf)), [], [])


def _refused(nf, host, rp, rt, edit):
    return cases.c_plan(nf, host, rp, rt, edit)[0]


def test_refusals():
    # three frames; p0, p1 hosted by 0, p2 by 1, p3 by 2.  p0 observes 1 and 2, p1 observes 1, p2 observes 0, p3 observes 0 and 1.
    nf, host = 3, [0, 0, 1, 2]
    rp, rt = [0, 0, 1, 2, 3, 3], [1, 2, 1, 0, 0, 1]
    ok = dict(drop_res=[0], remove_points=[1], drop_point=[0, 0, 0, 0], n_add_frames=1, add_res=[(0, 3)], add_points=[3], pt_res=[(0, 0)])
    assert _refused(nf, host, rp, rt, ok) == 0                                       # the base of the variations below is legal
    bad = {
        "res index out of range": dict(drop_res=[6]),
        "res index negative": dict(drop_res=[-1]),
        "res named twice": dict(drop_res=[2, 2]),
        "point index out of range": dict(remove_points=[4]),
        "point named twice": dict(remove_points=[1, 1]),
        "flagged after stage 2 removed it": dict(remove_points=[1], drop_point=[0, 1, 0, 0]),
        "frame index out of range": dict(remove_points=[0, 1], remove_frames=[3]),
        "frame named twice": dict(remove_points=[0, 1], remove_frames=[0, 0]),
        "frame still hosts a point": dict(remove_points=[0], remove_frames=[0]),
        "residual added to a point that leaves (stage 2)": dict(remove_points=[1], add_res=[(1, 2)]),
        "residual added to a point that leaves (stage 3)": dict(drop_point=[0, 1, 0, 0], add_res=[(1, 2)]),
        "residual onto its own host": dict(add_res=[(1, 0)]),
        "residual onto an observed target": dict(add_res=[(1, 1)]),
        "residual onto a target added in the same call": dict(add_res=[(1, 2), (1, 2)]),
        "residual into a frame that leaves": dict(remove_points=[0, 1], remove_frames=[0], add_res=[(3, 0)]),
        "residual target out of range": dict(add_res=[(1, 3)]),
        "residual point out of range": dict(add_res=[(4, 1)]),
        "new point hosted by a frame that leaves": dict(remove_points=[0, 1], remove_frames=[0], add_points=[0]),
        "new point's residual into a frame that leaves": dict(remove_points=[0, 1], remove_frames=[0], add_points=[1], pt_res=[(0, 0)]),
        "new point's residual onto its host": dict(add_points=[1], pt_res=[(0, 1)]),
        "new point observes a target twice": dict(add_points=[1], pt_res=[(0, 0), (0, 0)]),
        "new point's residuals not grouped": dict(add_points=[1, 2], pt_res=[(1, 0), (0, 0)]),
        "new point's residual names no point": dict(add_points=[1], pt_res=[(1, 0)]),
        "host of a new point out of range": dict(add_points=[3]),
        "more than 8 frames": dict(n_add_frames=6),
    }
    for why, edit in bad.items():
        assert _refused(nf, host, rp, rt, edit) == SDSO_ERR_ARG, why
        with pytest.raises(ValueError):
            ref.apply_edit(nf, host, rp, rt, edit)
    # A ninth residual: with at most 8 frames, no residual onto the host and no target twice, a point holds at most 7 residuals, so the
    # refusals above (own host, observed target, more than 8 frames) are what stands in front of MAX_RES_PER_POINT = 8.  A point that
    # observes all 7 other frames can swap two of them, and cannot gain one:
    nf, host, rp, rt = 8, [0], [0] * 7, list(range(1, 8))
    assert _refused(nf, host, rp, rt, dict(drop_res=[0, 1], add_res=[(0, 1), (0, 2)])) == 0
    assert _refused(nf, host, rp, rt, dict(n_add_frames=1, add_res=[(0, 8)])) == SDSO_ERR_ARG
    # a dropped residual's point may leave in a later stage: legal
    assert _refused(3, [0, 0, 1, 2], [0, 0, 1, 2, 3, 3], [1, 2, 1, 0, 0, 1], dict(drop_res=[2], remove_points=[1])) == 0
    assert _refused(3, [0, 0, 1, 2], [0, 0, 1, 2, 3, 3], [1, 2, 1, 0, 0, 1], dict(drop_res=[2], drop_point=[0, 1, 0, 0])) == 0


def test_counts_beyond_the_window_are_refused_before_anything_is_sized():
    """a count no window can hold is an argument error, not an allocation"""
    import ctypes as C
    from sdso_amd import abi
    L = abi.load()
    host = np.array([0, 0, 1, 2], np.int32); rp = np.array([0, 0, 1, 2, 3, 3], np.int32); rt = np.array([1, 2, 1, 0, 0, 1], np.int32)
    for field, value in (("n_add_frames", 2 ** 30), ("n_add_frames", 2 ** 31 - 1), ("n_add_points", 2 ** 31 - 1), ("n_drop_res", 7), ("n_pt_res", 2 ** 31 - 1)):
        E, keep = cases.to_abi({})
        setattr(E, field, value)
        n2 = C.c_int(0)
        assert L.sdso_ba_window_plan(3, 4, 6, abi.ip(host), abi.ip(rp), abi.ip(rt), C.byref(E), C.byref(n2), C.byref(n2), C.byref(n2), None, None, None) == SDSO_ERR_ARG, field
