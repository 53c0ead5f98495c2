"""Pins tests/window_edit_ref.py, the plain-Python statement of sdso_ba_window_update's seven stages, with cases derived by hand from the
reference's list operations (EnergyFunctional.cpp:524-533 dropResidual, :755-771 removePoint, :739-752 dropPointsF, :692-696).
Every expected value below was written down by hand, following the std::vector operations step by step; none is computed with the model."""
import itertools

import numpy as np
import pytest

import window_edit_ref as ref

A, B, C_, D, E_ = 0, 1, 2, 3, 4


def _one_host(n):
    """n points hosted by frame 0 of a two-frame window, no residuals"""
    return 2, [0] * n, [], []


def test_remove_point_one_after_the_other():
    # [a b c d e]: removePoint(a) -> [e b c d]; removePoint(b) -> [e d c]; removePoint(e) -> [c d]
    nf, host, rp, rt = _one_host(5)
    f, p, r = ref.apply_edit(nf, host, rp, rt, dict(remove_points=[A, B, E_]))
    assert (f, p, r) == ([0, 1], [C_, D], [])
    assert ref.remove_points_in_order([A, B, C_, D, E_], [A, B, E_]) == [C_, D]


def test_drop_points_rescanning_loop():
    # [a b c d e], a b e flagged: i=0 a -> [e b c d]; i=0 e -> [d b c]; i=0 d stays; i=1 b -> [d c]; i=1 c stays
    nf, host, rp, rt = _one_host(5)
    f, p, r = ref.apply_edit(nf, host, rp, rt, dict(drop_point=[1, 1, 0, 0, 1]))
    assert (f, p, r) == ([0, 1], [D, C_], [])
    assert ref.drop_points_rescan([A, B, C_, D, E_], [A, B, E_]) == [D, C_]


def test_the_two_point_removals_differ_in_29_of_254_subsets():
    """every subset of lists of 1..7 entries, stage 2 in ascending order against stage 3: the two procedures are not
    interchangeable (sum of 2^n for n = 1..7 is 254 cases)"""
    cases = differ = 0
    for n in range(1, 8):
        for mask in range(2 ** n):
            leaving = [i for i in range(n) if (mask >> i) & 1]
            cases += 1
            differ += ref.remove_points_in_order(range(n), leaving) != ref.drop_points_rescan(range(n), leaving)
    assert (cases, differ) == (254, 29)


def test_drop_residual_order_decides_the_list():
    # one point hosted by frame 4 with residuals [t0 t1 t2 t3] = ids 0..3
    nf, host, rp, rt = 5, [4], [0, 0, 0, 0], [0, 1, 2, 3]
    # drop t0: [t3 t1 t2]; drop t1: [t3 t2]
    assert ref.apply_edit(nf, host, rp, rt, dict(drop_res=[0, 1]))[2] == [3, 2]
    # drop t1: [t0 t3 t2]; drop t0: [t2 t3]
    assert ref.apply_edit(nf, host, rp, rt, dict(drop_res=[1, 0]))[2] == [2, 3]


def test_two_frames_leave_in_one_call():
    # the same point; frames 0 and 1 leave.  Frame 0 first: [r3 r1 r2] then frame 1: [r3 r2].  Frame 1 first: [r0 r3 r2] then frame 0: [r2 r3].
    nf, host, rp, rt = 5, [4], [0, 0, 0, 0], [0, 1, 2, 3]
    maps = ref.apply_edit(nf, host, rp, rt, dict(remove_frames=[0, 1]))
    assert maps == ([2, 3, 4], [0], [3, 2])
    h2, rp2, rt2 = ref.flatten(nf, host, rp, rt, dict(remove_frames=[0, 1]), maps)
    assert list(h2) == [2] and list(rp2) == [0, 0] and list(rt2) == [1, 0]          # old frames 2 3 4 are now 0 1 2
    maps = ref.apply_edit(nf, host, rp, rt, dict(remove_frames=[1, 0]))
    assert maps == ([2, 3, 4], [0], [2, 3])
    # two points, hosts 2 and 3 of four frames: p0 [r0>0 r1>1 r2>3], p1 [r3>0 r4>2 r5>1]
    nf, host, rp, rt = 4, [2, 3], [0, 0, 0, 1, 1, 1], [0, 1, 3, 0, 2, 1]
    # frame 0: p0 [r2 r1], p1 [r5 r4]; frame 1: p0 [r2], p1 [r4]
    maps = ref.apply_edit(nf, host, rp, rt, dict(remove_frames=[0, 1]))
    assert maps == ([2, 3], [0, 1], [2, 4])
    h2, rp2, rt2 = ref.flatten(nf, host, rp, rt, dict(remove_frames=[0, 1]), maps)
    assert list(h2) == [0, 1] and list(rp2) == [0, 1] and list(rt2) == [1, 0]


def test_appended_frame_with_a_new_residual_and_a_new_point():
    # two frames; p0 hosted by 0 observes 1 (r0), p1 hosted by 1 observes 0 (r1).  Frame 2 is appended; stage 6 gives p1 then p0 a
    # residual into it (ids -1, -2); stage 7 adds a point hosted by frame 2 (id -1) with residuals into 0 and 1 (ids -3, -4) and a point
    # hosted by frame 0 (id -2) with a residual into 2 (id -5).
    nf, host, rp, rt = 2, [0, 1], [0, 1], [1, 0]
    edit = dict(n_add_frames=1, add_res=[(1, 2), (0, 2)], add_points=[2, 0], pt_res=[(0, 0), (0, 1), (1, 2)])
    maps = ref.apply_edit(nf, host, rp, rt, edit)
    assert maps == ([0, 1, -1], [0, -2, 1, -1], [0, -2, -5, 1, -1, -3, -4])
    h2, rp2, rt2 = ref.flatten(nf, host, rp, rt, edit, maps)
    assert list(h2) == [0, 0, 1, 2] and list(rp2) == [0, 0, 1, 2, 2, 3, 3] and list(rt2) == [1, 2, 2, 0, 2, 0, 1]


def test_stages_run_in_order():
    # a residual dropped in stage 1 whose point leaves in stage 2 is legal; flagged (stage 3) after stage 2 removed it is not
    nf, host, rp, rt = 3, [0, 0, 1], [0, 0, 1, 2], [1, 2, 2, 0]
    assert ref.apply_edit(nf, host, rp, rt, dict(drop_res=[0], remove_points=[0])) == ([0, 1, 2], [1, 2], [2, 3])
    with pytest.raises(ValueError):
        ref.apply_edit(nf, host, rp, rt, dict(remove_points=[0], drop_point=[1, 0, 0]))
    with pytest.raises(ValueError):
        ref.apply_edit(nf, host, rp, rt, dict(remove_frames=[1]))                  # still hosts point 2
    assert ref.apply_edit(nf, host, rp, rt, {}) == ([0, 1, 2], [0, 1, 2], [0, 1, 2, 3])
