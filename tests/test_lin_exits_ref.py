"""What the every-exit window (tests/lin_exits_cases.py) must be, on the CPU oracle alone: the GPU test compares bit for bit and would
pass just as well on a window that no residual left early.  The counts are conditions on the input, not tolerances on any output."""
import numpy as np
import pytest

import lin_exits_cases as Lx


@pytest.fixture(scope="module")
def case(oracle):
    win = Lx.window()
    return win, Lx.oracle_rounds(oracle, win), Lx.oracle_rounds(oracle, win, new_frame_th=False)


def test_oracle_takes_every_exit(case):
    win, (o1, o2), _ = case
    nr = win["nr"]
    sticky = Lx.preset_sticky(nr)
    assert win["np"] == 240 and nr == 627
    ns = o1["ns"]
    print("round 1: IN %d OUTLIER %d OOB %d (preset-sticky %d, fresh %d)" % ((ns == 0).sum(), (ns == 2).sum(), (ns == 1).sum(),
                                                                          (sticky & (ns == 1)).sum(), (~sticky & (ns == 1)).sum()))
    assert ((ns == 0).sum(), (ns == 2).sum(), (ns == 1).sum()) == (232, 267, 128)
    assert sticky.sum() == 57 and (ns[sticky] == 1).all() and (~sticky & (ns == 1)).sum() == 71
    assert np.array_equal(o1["nw"] == -1, ns == 1)               # state_NewEnergyWithOutlier stays -1 on exactly the OOB residuals
    # which exit each fresh one took, in float64 from the window's own poses and idepths
    ex = Lx.classify_exits(win)
    n = {name: int((ex == k).sum()) for k, name in enumerate(Lx.EXITS)}
    print("exits of the residuals that are not preset-sticky:", n)
    assert n["drescale"] >= 5 and n["centre"] >= 5 and n["pattern"] >= 5 and sticky.sum() >= 5
    assert np.array_equal((ex >= 0) & (ex < 3), ~sticky & (ns == 1))   # ... and the oracle left through an exit exactly there
    assert n["ran"] == (ns != 1).sum()


@pytest.mark.parametrize("new_frame_th", [True, False])
def test_second_round_is_sticky(case, new_frame_th):
    win, (o1, o2) = case[0], case[1 if new_frame_th else 2]
    oob1 = o1["ns"] == 1
    assert np.array_equal(o1["st"], o1["ns"]) and oob1.sum() >= 128
    assert (o2["ns"][oob1] == 1).all() and (o2["nw"][oob1] == -1).all() and (o2["st"][oob1] == 1).all() and (o2["act"][oob1] == 0).all()
    print("round 2: IN %d OUTLIER %d OOB %d" % ((o2["ns"] == 0).sum(), (o2["ns"] == 2).sum(), (o2["ns"] == 1).sum()))
    assert (o2["ns"] == 1).sum() == oob1.sum() and (o2["act"] == 1).sum() > 200 and (o2["ns"] == 2).sum() > 100
    if not new_frame_th:                                         # same thresholds, same inputs: the same decisions
        assert np.array_equal(o2["ns"], o1["ns"]) and np.array_equal(o2["ne"], o1["ne"])
    else:
        assert (o2["ns"] != o1["ns"]).sum() >= 50                # the new threshold moves residuals between IN and OUTLIER
