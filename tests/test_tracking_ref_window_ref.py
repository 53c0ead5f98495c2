"""tests/tracking_ref_window_ref.py against a hand-written window: which points makeCoarseDepthL0 STEP1 uses (CoarseTracker.cpp:295)."""
import numpy as np
import pytest

from tracking_ref_window_ref import IN, OOB, OUTLIER, expected_points

# 3 keyframes (newest = 2), 7 points.  One row per residual: (point, target, state_state, isActiveAndIsGoodNEW)
RES = [
    (0, 1, IN, 1), (0, 2, IN, 1),              # point 0: IN into the newest frame                        -> used
    (1, 1, IN, 1),                             # point 1: no residual into the newest frame               -> not used
    (2, 2, OUTLIER, 0), (2, 1, IN, 1),         # point 2: its residual into the newest frame is OUTLIER   -> not used
    (3, 2, OOB, 0),                            # point 3: ... OOB                                         -> not used
    (4, 0, IN, 1), (4, 2, IN, 0),              # point 4: ... IN before, on toRemove now (.first cleared) -> not used
    (5, 2, IN, 1), (5, 0, OUTLIER, 0),         # point 5: IN into the newest; the OUTLIER elsewhere does not matter -> used
    (6, 0, IN, 1), (6, 1, IN, 1), (6, 2, IN, 1),   # point 6 (hosted by nobody special), residualsAll not in target order -> used
]
POINT, TARGET, STATE, ACT = [np.array(c) for c in zip(*RES)]


def test_window_order():
    got = expected_points(STATE, ACT, TARGET, POINT, newest=2)
    assert got.dtype == np.int32 and got.tolist() == [0, 5, 6]


def test_permuted_order_is_kept_and_restricted():
    assert expected_points(STATE, ACT, TARGET, POINT, newest=2, order=[6, 3, 0, 2, 5, 4, 1]).tolist() == [6, 0, 5]
    assert expected_points(STATE, ACT, TARGET, POINT, newest=2, order=[5, 1, 6]).tolist() == [5, 6]       # point 0 is left out by the caller


def test_another_newest_frame_and_an_empty_window():
    assert expected_points(STATE, ACT, TARGET, POINT, newest=1).tolist() == [0, 1, 2, 6]
    assert expected_points([], [], [], [], newest=2, n_points=3).tolist() == []


def test_bad_inputs_are_refused():
    with pytest.raises(AssertionError):
        expected_points(STATE, ACT, TARGET, POINT, newest=2, order=[0, 0, 1])
    with pytest.raises(AssertionError):
        expected_points([IN, IN], [1, 1], [2, 2], [0, 0], newest=2)
