"""CPU checks behind tests/test_full_window_gpu.py, on the oracle and the CPU statements alone: the conditions that keep the GPU
comparisons at the full window from passing vacuously.  Every figure is printed before it is asserted."""
import copy

import numpy as np
import pytest

import activate_ref as AR
import distmap_ref as D
import full_window_cases as FW
import immature_ref as R


@pytest.fixture(scope="module")
def ran(oracle):
    return {name: FW.run_oracle(oracle, FW.batch(name)) for name in FW.BATCH_NAMES}


@pytest.mark.parametrize("name", ["nf8", "nf8_minobs7", "nf7", "nf3", "nf2", "nf8_all_but_3"])
def test_batch_case_reaches_every_status_on_every_host(ran, name):
    d = FW.batch(name)["d"]
    st = ran[name][0]
    per_host = [int(((d["host"] == h) & (st == 1)).sum()) for h in range(d["nf"])]
    print(name, "n", len(st), "statuses -1/0/1", [int((st == s).sum()) for s in (-1, 0, 1)], "activated per host", per_host)
    assert set(np.unique(st)) == {-1, 0, 1}
    assert min(per_host) >= 1


def test_batch_sizes_cover_every_remainder_of_the_four_waves_of_a_block(ran):
    n = {name: len(ran[name][0]) for name in FW.BATCH}
    print(n)
    assert {v % 4 for v in n.values()} == {0, 1, 2, 3}
    assert n["nf8_first_point"] == 1 and n["nf8_all_but_3"] == n["nf8"] - 3 and n["nf8"] % 4 == 0


def test_every_residual_slot_shows_every_state_at_nf8(ran):
    d = FW.batch("nf8")["d"]
    st, _, rs = ran["nf8"]
    slots = FW.slot_states(d, rs)[st != 0]
    table = np.array([[int((slots[:, s] == k).sum()) for k in (0, 1, 2)] for s in range(7)])
    print("slot x (IN, OOB, OUTLIER):\n", table)
    assert (table >= 1).all()
    assert set(np.unique(d["host"][st != 0])) == set(range(8))


def test_min_obs_7_rejects_points_that_min_obs_2_activates(ran):
    s2, s7 = ran["nf8"][0], ran["nf8_minobs7"][0]
    print("minObs 2:", [int((s2 == s).sum()) for s in (-1, 0, 1)], "minObs 7:", [int((s7 == s).sum()) for s in (-1, 0, 1)])
    assert ((s2 == 1) & (s7 == -1)).sum() >= 1
    assert np.array_equal(s2 == 0, s7 == 0)


def test_the_eighth_keyframe_changes_the_result(oracle, ran):
    """the same points in the window without its last keyframe: a kernel that mishandles the seventh residual cannot be bit-exact at nf = 8"""
    case = FW.batch("nf8")
    d7 = FW.without_last_frame(case["d"])
    s7, i7, _ = FW.run_oracle(oracle, case, d=d7)
    keep = case["d"]["host"] < 7
    s8, i8 = ran["nf8"][0][keep], ran["nf8"][1][keep]
    both = (s7 == 1) & (s8 == 1)
    changed = int((i7[both] != i8[both]).sum())
    print("activate both ways", int(both.sum()), "idepth differs", changed)
    assert both.sum() >= 100 and 2 * changed >= both.sum()


def test_crafted_case_fails_first_at_every_pattern_pixel(ran):
    case = FW.crafted()
    first, clear = FW.first_failing(case["d"], case["imgs"][2])
    st, _, rs = ran["crafted"]
    print("first failing pixel", first.tolist(), "\nclearance min", float(clear.min()), "\nstatus", st.tolist())
    assert np.array_equal(first, case["want_first"])
    assert clear.min() >= FW.CLEARANCE                         # rounding cannot move a decision
    assert set(first) == set(range(8))
    slot2 = FW.slot_states(case["d"], rs)[:, 1]
    assert (slot2[st != 0] == 1).all()                         # and the oracle agrees: out of bounds in frame 2
    for k in range(1, 8):
        assert (st[first == k] == 1).any(), k


def test_crafted_case_depends_on_the_pixels_before_the_failing_one(oracle, ran):
    """the same points with frame 2 out of bounds from the first pixel on: if the result did not change, dropping the contributions of the
    pixels before the failing one would go unnoticed"""
    case = FW.crafted()
    first, _ = FW.first_failing(case["d"], case["imgs"][2])
    d = dict(case["d"], pair_t=case["d"]["pair_t"].copy())
    for host in (0, 1):
        d["pair_t"][host * 3 + 2] *= np.float32(1e4)
    first_far, _ = FW.first_failing(d, case["imgs"][2])
    assert (first_far == 0).all()
    _, idp_far, _ = FW.run_oracle(oracle, case, d=d)
    changed = [int((idp_far[first == k] != ran["crafted"][1][first == k]).sum()) for k in range(8)]
    print("idepth changes per first failing pixel", changed)
    assert changed[0] == 0 and min(changed[1:]) >= 1


@pytest.fixture(scope="module")
def resident(oracle):
    c = FW.resident()
    before = [len(g["u"]) for g in c["win"]["groups"][:7]]
    r = AR.activate(oracle, c["win"], FW.ref_map(c), 2, c["min_act_dist"])
    return c, before, r


def test_resident_window_selects_more_than_the_first_copy(resident):
    c, before, r = resident
    first_copy = FW.abi_define("SDSO_IMM_ACT_FIRST_COPY")
    st = r["records"]["status"]
    rows = np.bincount(r["row"], minlength=6)
    after = r["counts"][9:16]
    print("first copy", first_copy, "counts", r["counts"].tolist(), "rows", rows.tolist(), "before", before)
    assert FW.abi_define("SDSO_IMM_MAX_HOSTS") == 8 and len(c["before_key"]) == 8 and len(c["newest"]["u"]) > 0
    assert r["counts"][3] > first_copy and r["counts"][4] == r["counts"][3]
    assert (rows >= 5).all()                                                       # each of distmap_ref.select's six rows
    sel_per_group = np.bincount(r["records"]["frame"], minlength=7)
    print("selected per group", sel_per_group.tolist(), "lost per group", [b - int(a) for b, a in zip(before, after)])
    assert (sel_per_group >= 1).all() and all(int(a) < b for a, b in zip(after, before))
    assert all((st == s).sum() >= 1 for s in (-1, 0, 1))
    oob = r["records"]["lastTraceStatus"] == R.OOB
    assert ((st == 0) & oob).sum() >= 1 and ((st == 0) & ~oob).sum() >= 1
    late = np.arange(len(st)) >= first_copy
    opt = np.nonzero(r["decision"] == D.SELECT)[0]
    assert (st[late] == 1).any() and r["flags"][opt[late]].any()


def test_the_key_trace_reaches_all_eight_groups(oracle):
    c = FW.resident(doctored=False)
    r = AR.activate(oracle, copy.deepcopy(c["win"]), FW.ref_map(c), 2, c["min_act_dist"])
    print("the traced set as it is: counts", r["counts"].tolist())
    assert r["counts"][4] > FW.abi_define("SDSO_IMM_ACT_FIRST_COPY")
    changed = [R.same(a, b) is not None for a, b in zip(c["before_key"], c["win"]["groups"][:7] + [c["newest"]])]
    print("key trace counts", c["key_counts"].tolist())
    assert all(changed)
    assert (c["newest"]["lastTraceStatus"] == R.GOOD).sum() >= 10
