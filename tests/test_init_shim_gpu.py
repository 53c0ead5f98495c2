"""sdso_shim::CoarseInitializer (host/sdso_shim.h) driven by host/test_init_shim.cpp on stand-in types: setFirstStereo and
initializeFromInitializer with the process's real rand(), against the two reference loops written out over the C-ABI's older entry points
in the same program.  Pnts, points, their order and the members the callers read are identical, and the process's rand() stream stands
where the reference's local PixelSelector leaves it."""
import numpy as np
import pytest

import init_cases as IC
import shim_driver

f32 = np.float32
W, H = IC.SIZES[0]


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_init_shim")


def test_init_shim_driver_compiles():
    """CPU: the shim's CoarseInitializer class + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_init_shim")


@pytest.mark.gpu
def test_shim_start_equals_the_restated_reference_loops(driver, tmp_path):
    P = IC.stereo_pair(W, H)
    K4 = P["K4"]
    arrays = dict(meta=np.array([W, H, 3], np.int32), calib=np.array([K4[0], K4[1], K4[2], K4[3], P["baseline"], IC.DESIRED_POINT_DENSITY], f32), right=P["right"])
    for l in range(3):
        arrays["left_dI%d" % l] = P["pyr_left"][l]
    r = shim_driver.run("test_init_shim", tmp_path, arrays, mode="run")
    out = r.out
    draw_shim, draw_ref, after_shim, after_ref, made, nl = out("draws", np.int32)
    # the next rand() after setFirstStereo is the one after srand(3141592) and w*h draws; STEP 3 then drew once per Pnt on both routes
    assert draw_shim == draw_ref and after_shim == after_ref
    members = list(out("members", np.int32))
    assert members == [nl, 0, 0, 0, 1, 1], members                                   # numPoints[0], frameID, snapped, snappedAt, firstFrame, firstRightFrame
    assert np.array_equal(out("thisToNext", np.float64), np.concatenate([np.eye(3).ravel(), np.zeros(3)]))
    assert made == 9205 and nl == 9205                                                # the 640 x 480 case of tests/test_init_ref.py
    a, b = out("shim_pnts", np.uint32).reshape(-1, 7), out("ref_pnts", np.uint32).reshape(-1, 7)
    assert a.shape == (nl, 7) and np.array_equal(a, b)                                # as bits
    pa, pb = out("shim_points", np.uint32).reshape(-1, 24), out("ref_points", np.uint32).reshape(-1, 24)
    assert np.array_equal(pa, pb)
    n = len(pa)
    assert 0.1 * nl < n < 0.3 * nl and (np.diff(pa[:, 0].astype(np.int64)) > 0).all()   # sub-selected by rand(), in Pnt order
    pn = a.view(f32)
    assert (pn[:, 5] == 8 * 144.0).all() and (pn[:, 6] == 1).all() and (pn[:, 2] == f32(0.01)).sum() > 100
    assert r.stdout.split() == ["pnts", str(nl), str(nl), "points", str(n), str(n)]
