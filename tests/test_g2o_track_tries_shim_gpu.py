"""sdso_shim::CoarseTracker::trackNewCoarse with forkLive = true (host/shim/tracker.h) on the stand-in types —
host/test_g2o_track_tries_shim.cpp — against sdso_g2o_track_new_coarse through the C-ABI from Python, for the lists [H, H, G], [G, H, H]
and [H, H] of tests/test_g2o_track_tries_gpu.py run one after the other on ONE tracker: the same library and the same calls, so every
output is equal; firstCoarseRMSE is set by the first list (FullSystem.cpp:528-529) and left alone by the others; lastTries is filled."""
import numpy as np
import pytest

import helpers
import shim_driver
import track_tries_cases as cases
import track_tries_ref as ref
import g2o_track_tries_cases as g2o

DRIVER = "test_g2o_track_tries_shim"


def test_g2o_track_tries_driver_compiles():
    """CPU: the member and its driver compile against the ABI header with the plain host compiler"""
    shim_driver.rebuild(DRIVER)


@pytest.mark.gpu
def test_shim_fork_live_track_new_coarse(gpu_ctx, tmp_path):
    prob = cases.problem()
    L = prob["levels"]
    prm = helpers.track_params(prob)
    gpu_ctx.upload_pyramid(cases.NEW_SLOT, prob["pyr_new"]); gpu_ctx.set_ref(cases.REF_SLOT, prob["pc"])
    lists = [([cases.H, cases.H, cases.G], (0.0, 0.0), 1e9), ([cases.G, cases.H, cases.H], (0.0, 0.0), 0.0), ([cases.H, cases.H], (0.03, -1.5), 1e9)]
    thr = 1.5
    want = []
    for xs, aff0, rm in lists:
        rc, out, rmse, R = g2o.new_coarse(gpu_ctx, prm, cases.poses(xs), aff0, [rm] * 5, thr)
        gpu_ctx.check(rc)
        want.append((out, rmse, R))
    arrays = dict(meta=np.array([L, 640, 480, prm.coarsestLvl, len(lists)], np.int32), calib=np.array(prob["K"], np.float64),
                  misc=np.array([1.0, 1.0, 0.0, 0.0, thr], np.float64),
                  ntries=np.array([len(xs) for xs, _, _ in lists], np.int32),
                  tries=np.array([p for xs, _, _ in lists for p in cases.poses(xs)], np.float64),
                  aff0=np.array([a for _, a, _ in lists], np.float64), rmse=np.array([[rm] * 5 for _, _, rm in lists], np.float64))
    for l in range(L):
        arrays["ref_l%d" % l] = prob["pyr_ref"][l]; arrays["new_l%d" % l] = prob["pyr_new"][l]
        for k in ("u", "v", "idepth", "color"):
            arrays["pc_%s_l%d" % (k, l)] = prob["pc"][l][k]
    shim_driver.build(DRIVER)
    r = shim_driver.run(DRIVER, tmp_path, arrays)
    assert r.lines[-1] == "g2o_track_tries_shim ok: %d lists" % len(lists)
    ints = r.out("ints", np.int32).reshape(len(lists), 3)
    dbl = r.out("doubles", np.float64).reshape(len(lists), 36)
    per_try = r.out("per_try", np.int32).reshape(-1, 4)
    same = lambda a, b: len(a) == len(b) and all(ref.same_double(float(x), float(y)) for x, y in zip(a, b))   # noqa: E731
    t0 = 0
    for k, (out, rmse, R) in enumerate(want):
        assert list(ints[k]) == [out.haveOneGood, out.winner, out.tryIterations], k
        d = dbl[k]
        assert same(d[0:12], cases.se3_tuple(out.pose)) and same(d[12:14], (out.aff.a, out.aff.b)), k
        assert same(d[14:17], out.flowVecs[:]) and same(d[17:22], out.achievedRes[:]) and same(d[22:27], rmse), k
        last = R[out.tryIterations - 1]
        assert same(d[27:32], last.lastResiduals[:]) and same(d[32:35], last.lastFlowIndicators[:]), k
        assert ref.same_double(float(d[35]), want[0][0].achievedRes[0]), k        # firstCoarseRMSE: set once, by the first list
        n = len(R)
        assert [list(x) for x in per_try[t0:t0 + n]] == [[R[i].ran, R[i].good, R[i].abort_lvl, R[i].winner] if R[i].ran else [0, 0, 0, 0] for i in range(n)], k
        t0 += n
    assert len(per_try) == t0                                                     # lastTries: one record per try of every list
    assert [w[0].winner for w in want] == [2, 0, -1] and np.isfinite(dbl[0, 35])
