"""CPU checks of the stereoMatch statement (tests/stereo_match_ref.py): the case exercises every branch of the accept rule, and the
vectorised statement equals a plain per-point loop over the same oracle outputs.  tests/test_stereo_match_gpu.py holds the device to this
statement on this case."""
import numpy as np
import pytest

import immature_ref as R
import stereo_match_cases as Ms
import stereo_match_ref as M

f32 = np.float32


@pytest.fixture(scope="module")
def stated(oracle):
    c = Ms.pair()
    S = R.add_frame(oracle, c["left"], c["maps"][1037])
    before = {k: np.array(v, copy=True) for k, v in S.items()}
    return c, S, before, M.stereo_match(oracle, S, c["left"], c["right"], c["K4"], c["baseline"])


def test_case_covers_every_branch_of_the_rule(stated):
    c, S, before, r = stated
    cn = r["counts"]
    print("counts", cn, "forward", np.bincount(r["status_fwd"], minlength=6)[:6], "back", np.bincount(r["status_back"][r["status_back"] != M.NOT_RUN], minlength=6)[:6])
    assert len(S["u"]) == 1037 and cn[M.C_WALKED] == 1037
    assert cn[M.C_ACCEPTED] >= 500 and cn[M.C_FAR] >= 50 and cn[M.C_DEPTH] >= 5
    assert (r["status_fwd"] != R.GOOD).sum() >= 1
    ran = r["status_back"] != M.NOT_RUN
    assert (r["status_back"][ran] != R.GOOD).sum() >= 1
    assert cn[M.C_BACK_GOOD] == cn[M.C_ACCEPTED] + cn[M.C_FAR] + cn[M.C_DEPTH]
    assert cn[M.C_UNREADABLE] == 0 and cn[M.C_BACK_RUN] == cn[M.C_FWD_GOOD] == (r["status_fwd"] == R.GOOD).sum()
    assert R.same(S, before) is None                                   # the statement leaves the group alone


def test_statement_equals_a_per_point_loop(stated):
    """:598-611 written as the reference writes it, one point at a time, on the traces' raw outputs"""
    c, S, before, r = stated
    h, w, _ = c["left"].shape
    m = np.zeros((h, w, 3), f32)
    counter = 0
    acc = np.zeros(len(S["u"]), np.uint8)
    idepth = np.zeros((len(S["u"]), 3), f32)
    with np.errstate(all="ignore"):
        for i in range(len(S["u"])):
            if r["status_fwd"][i] != R.GOOD or r["status_back"][i] == M.NOT_RUN:
                continue
            u_stereo_delta = abs(f32(S["u"][i]) - f32(r["back_u"][i]))
            depth = f32(1.0) / f32(r["fwd"][i, 0])
            if r["status_back"][i] == R.GOOD and u_stereo_delta < 1 and depth > 0 and depth < 70:
                m[int(S["v"][i]), int(S["u"][i])] = r["fwd"][i]
                idepth[i] = r["fwd"][i]
                acc[i] = 1
                counter += 1
    assert counter == r["counts"][M.C_ACCEPTED]
    assert np.array_equal(acc, r["accepted"]) and np.array_equal(idepth, r["idepth"]) and np.array_equal(m, r["map"])
    assert (m[..., 0] != 0).sum() == counter                           # one point per pixel, every accepted idepth_stereo non-zero
    assert (idepth[acc == 0] == 0).all() and np.isfinite(idepth).all()


@pytest.mark.parametrize("n", [259, 1, 0])
def test_smaller_groups(oracle, n):
    c = Ms.pair()
    S = R.add_frame(oracle, c["left"], c["maps"][n])
    r = M.stereo_match(oracle, S, c["left"], c["right"], c["K4"], c["baseline"])
    cn = r["counts"]
    print(n, "counts", cn)
    assert cn[M.C_WALKED] == n == len(S["u"])
    assert cn[M.C_ACCEPTED] == r["accepted"].sum() == (r["map"][..., 0] != 0).sum() and cn[M.C_ACCEPTED] >= min(n, 100)
    assert cn[M.C_BACK_GOOD] == cn[M.C_ACCEPTED] + cn[M.C_FAR] + cn[M.C_DEPTH] and cn[M.C_UNREADABLE] == 0
    if n == 0:
        assert not r["map"].any()


def test_max_depth_moves_points_between_two_counts(stated, oracle):
    c, S, before, r = stated
    r20 = M.stereo_match(oracle, S, c["left"], c["right"], c["K4"], c["baseline"], max_depth=20.0)
    moved = r["counts"][M.C_ACCEPTED] - r20["counts"][M.C_ACCEPTED]
    assert moved > 0 and r20["counts"][M.C_DEPTH] - r["counts"][M.C_DEPTH] == moved
    assert np.array_equal(np.delete(r["counts"], [M.C_ACCEPTED, M.C_DEPTH]), np.delete(r20["counts"], [M.C_ACCEPTED, M.C_DEPTH]))
