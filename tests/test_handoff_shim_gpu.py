"""The threaded binding of INTEGRATION.md §2 through the shim (host/test_handoff_shim.cpp on stand-in types): a mapping thread on one
sdso_shim::Device builds a tracking template per keyframe from the device-resident BA window and hands it over with
CoarseTracker::exportRef(); a tracking thread on a second Device adopts it (adoptRef) and tracks three frames whose pyramids it imports
from the mapper's Device, while the mapper is already building the next template and has released the last keyframe's frames and window.
The program then runs the same schedule on ONE Device in one thread and compares: every pose, affine pair, residual and iteration count
must be bit-equal — the hand-off computes nothing, it only decides who may read and write what, and when.

Six independent 320 x 240 windows (tracking_ref_window_cases.make_case, seeds 3101 + k), 3 optimisation steps each."""
import os

import numpy as np
import pytest

import shim_driver
import tracking_ref_window_cases as TC

K, ITS, TRACKED, REC = 6, 3, 3, 26
NF = 4


def _arrays(case):
    """window `case` as the files host/driver_io.h's WindowGraph reads (the right image of the newest keyframe as frame nf)"""
    arrays = dict(meta=np.array([case["nf"], case["np"], case["nr"], case["w"], case["h"], ITS, case["solverMode"], case["levels"]], np.int32),
                  calib=np.concatenate([case["calib_value_scaled"], case["calib_value_zero"], [case["baseline"]]]).astype(np.float64))
    for k, dt in (("evalPT", np.float64), ("state", np.float64), ("state_zero", np.float64), ("ab_exposure", np.float32), ("frameEnergyTH", np.float32),
                  ("frameID", np.int32), ("res_point", np.int32), ("res_target", np.int32), ("host", np.int32), ("u", np.float32), ("v", np.float32),
                  ("idepth", np.float32), ("idepth_zero", np.float32), ("color", np.float32), ("weights", np.float32), ("hasDepthPrior", np.uint8),
                  ("res_state", np.uint8)):
        arrays[k] = np.ascontiguousarray(case[k], dt)
    for f, pyr in enumerate(list(case["pyrs"]) + [case["pyr_right"]]):
        for l, img in enumerate(pyr):
            arrays["img%d_l%d" % (f, l)] = np.ascontiguousarray(img, np.float32)
    return arrays


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_handoff_shim")


def test_handoff_shim_driver_compiles():
    """CPU: Shared, exportFrame / importFrame, exportRef / adoptRef and the driver compile against the ABI header with the host compiler."""
    shim_driver.rebuild("test_handoff_shim")


@pytest.mark.gpu
def test_two_threads_two_devices_equal_one(driver, tmp_path):
    cases = [dict(nf=NF, pts_per_kf=200, seed=3101 + k) for k in range(K)]
    arrays = dict(meta=np.array([K, NF, ITS], np.int32))
    for k, case in enumerate(TC.make_case(**spec) for spec in cases):
        os.makedirs(str(tmp_path / ("k%d" % k)))
        for name, a in _arrays(case).items():
            arrays["k%d/%s" % (k, name)] = a
    r = shim_driver.run("test_handoff_shim", tmp_path, arrays, timeout=60)
    assert "handoff ok" in r.stdout
    two, one = r.out("two", np.float64).reshape(K * TRACKED, REC), r.out("one", np.float64).reshape(K * TRACKED, REC)
    assert two.tobytes() == one.tobytes()                                 # poses, affine pairs, lastResiduals, iteration counts
    assert np.array_equal(two[:, 24], np.repeat(1000 * np.arange(K) + 100 + NF - 1, TRACKED))     # refFrameID follows k
    assert (two[:, 19:24].sum(axis=1) > 0).all() and np.isfinite(two[:, :14]).all()               # every frame was iterated on
    assert len({two[i, :12].tobytes() for i in range(K * TRACKED)}) == K * TRACKED                # ... and each is a problem of its own
