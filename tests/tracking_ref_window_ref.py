"""Which points CoarseTracker::makeCoarseDepthL0 STEP1 splats, and in which order, stated on the post-state arrays of a window.

Reference (src/FullSystem/CoarseTracker.cpp:288-300): for every frame, for every pointHessian, the point is used iff
lastResiduals[0].first != 0 && lastResiduals[0].second == ResState::IN.  lastResiduals[0] is the point's residual into the newest
keyframe (FullSystem::makeKeyFrame gives every point one, FullSystem.cpp:1370-1387); the closing linearizeAll(true) of
FullSystem::optimize clears .first of a residual it puts on toRemove (FullSystemOptimize.cpp:176-195) and writes the final state into
.second (:165-172).  On the arrays of sdso_ba_get_post_state, in the window's residual order:

    selected(point) <=> one of its residuals has res_target == newest, isActiveAndIsGoodNEW != 0 (it is not on toRemove) and
                        state_state == IN

A point has at most one residual into a frame.  The splat order is the caller's order (FrameHessian::pointHessians order, frame by
frame) restricted to the selected points; without one it is the window's point order."""
import numpy as np

IN, OOB, OUTLIER = 0, 1, 2        # ResState, Residuals.h:49


def expected_points(state_state, isActiveAndIsGoodNEW, res_target, res_point, newest, order=None, n_points=None):
    """-> int32 array of window point indices, in splat order.
    state_state, isActiveAndIsGoodNEW, res_target, res_point: per residual, window order; newest: index of the newest keyframe (nf - 1);
    order: window point indices in the caller's order (each at most once; points it leaves out are not splatted), None: 0 .. n_points-1."""
    state_state = np.asarray(state_state)
    act = np.asarray(isActiveAndIsGoodNEW)
    res_target = np.asarray(res_target)
    res_point = np.asarray(res_point, np.int64)
    if n_points is None:
        n_points = int(res_point.max()) + 1 if len(res_point) else 0
    hit = (res_target == newest) & (act != 0) & (state_state == IN)
    per_point = np.bincount(res_point[res_target == newest], minlength=n_points) if len(res_point) else np.zeros(n_points, np.int64)
    assert per_point.max(initial=0) <= 1, "a point observes a frame at most once"
    selected = np.zeros(n_points, bool)
    selected[res_point[hit]] = True
    order = np.arange(n_points) if order is None else np.asarray(order, np.int64)
    assert len(np.unique(order)) == len(order), "a point is named at most once"
    return order[selected[order]].astype(np.int32)
