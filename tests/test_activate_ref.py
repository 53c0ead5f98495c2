"""CPU checks behind tests/test_imm_activate_gpu.py: the closed form of the STEP 5 removal order that the device computes, against the
reference's loop, and the conditions on the CPU statement's output that keep the GPU tests from passing vacuously — a later edit of the
case cannot hollow them out unnoticed."""
import itertools

import numpy as np
import pytest

from sdso_amd import abi
import activate_cases as AC
import activate_ref as AR
import immature_ref as R


def test_closed_form_of_the_removal_order():
    for n in range(0, 13):                                             # every flag pattern up to n = 12
        for bits in itertools.product((0, 1), repeat=n):
            assert AR.closed_form_order(bits) == R.remove_order(list(bits)), bits
    rs = np.random.RandomState(5)
    for k in range(2700):
        n = int(rs.randint(1, 1038))
        flags = (rs.rand(n) < rs.choice([0.02, 0.3, 0.7, 0.98])).astype(np.uint8)
        if k % 9 == 0:
            flags[-int(rs.randint(1, min(n, 40) + 1)):] = 1            # a run at the back
        assert AR.closed_form_order(flags) == R.remove_order(list(flags)), k


@pytest.fixture(scope="module")
def ran(oracle):
    out = {}
    for min_obs in (1, 2):
        c = AC.window(oracle)
        _, m = AC.ref_map(c)
        before = [len(g["u"]) if g is not None else 0 for g in c["win"]["groups"]]
        out[min_obs] = (AR.activate(oracle, c["win"], m, min_obs, c["min_act_dist"]), before, c)
    return out


def test_case_reaches_every_branch(ran):
    r, before, c = ran[2]
    rows = np.bincount(r["row"], minlength=6)
    st, lts = r["records"]["status"], r["records"]["lastTraceStatus"]
    oob = lts == R.OOB
    print("rows", rows, "statuses -1/0/1", [(st == s).sum() for s in (-1, 0, 1)], "status 0 with / without OOB", ((st == 0) & oob).sum(), ((st == 0) & ~oob).sum(),
          "counts", r["counts"])
    assert (rows >= 5).all()                                           # each of distmap_ref.select's six rows
    assert all((st == s).sum() >= 10 for s in (-1, 0, 1))
    assert ((st == 0) & oob).sum() >= 5 and ((st == 0) & ~oob).sum() >= 5
    after = r["counts"][9:9 + 4]
    assert sum(a < b for a, b in zip(after, before)) >= 2              # at least two hosts lose points
    ns = int(r["counts"][4])
    assert ns % 4 != 0 and ns % 64 != 0
    assert r["counts"][8] == sum(before) - after.sum() and r["counts"][0] == sum(before[:3])
    assert list(before) == [1037, 259, 1, 0]


def test_min_obs_changes_the_outcome(ran):
    """minObs = 1 (what the reference passes) and 2 decide differently for some points, so the GPU test that runs both checks both."""
    s1, s2 = ran[1][0]["records"]["status"], ran[2][0]["records"]["status"]
    assert len(s1) == len(s2) and (s1 != s2).sum() >= 1
    assert np.array_equal(ran[1][0]["decision"], ran[2][0]["decision"])
