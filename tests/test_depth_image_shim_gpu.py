"""sdso_shim::CoarseTracker::debugPlotIDepthMap / debugPlotIDepthMapFloat (host/sdso_shim.h) driven by host/test_depth_image_shim.cpp
on stand-in types: after setCoarseTrackingRef on the device-resident window, the two members push a B3 image and a float image to a
recording wrapper.  What the wrapper received equals the C-ABI's results on the same window, byte for byte; *minID_pt / *maxID_pt move as
the reference moves them; a tracker told of a one-level frame (w[1] == 0) pushes nothing."""
import numpy as np
import pytest

from sdso_amd import abi
import shim_driver
import tracking_ref_window_cases as TC
from test_tracking_ref_shim_gpu import ITS, _arrays


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_depth_image_shim")


def test_depth_image_shim_driver_compiles():
    """CPU: the two members and the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_depth_image_shim")


@pytest.mark.gpu
def test_pushed_images_equal_the_c_abi(driver, tmp_path):
    case = TC.make_case(nf=4, pts_per_kf=200, seed=3101)
    w, h = case["w"], case["h"]
    # ---- the C-ABI from Python on the same window, in a context of its own (the switch is per context)
    ctx = abi.Context(0)
    try:
        ctx.keep_depth_map(True)
        up = TC.upload(ctx, case, 78, 800)
        TC.optimize(ctx, up["wid"], ITS)
        _, pcn, _ = TC.window_route(ctx, up, 97)
        assert pcn[0] > 100
        first = ctx.depth_image(97, up["left"], w, h, (-1, -1))
        second = ctx.depth_image(97, up["left"], w, h, first["range"])
        third = ctx.depth_image(97, up["left"], w, h, None)
    finally:
        ctx.close()
    assert first["counts"][0] > 100 and first["counts"][1] > 100
    # ---- the driver
    arrays = _arrays(case, (-1, -1))
    r = shim_driver.run("test_depth_image_shim", tmp_path, arrays, "frame")
    info = r.out("frame_info", np.int32)
    assert list(info) == [3, 2, 1, 1, 1, w, h], info       # 3 B3 pushes, 2 float pushes, both wrappers alike, KF = lastRef, the map wrapped not copied
    for i, want in enumerate((first, second, third)):
        assert np.array_equal(r.out("frame_b3_%d" % i, np.uint8), want["rgb"].reshape(-1)), i
    for i in range(2):
        assert np.array_equal(r.out("frame_f_%d" % i, np.uint32), first["idepth"].view(np.uint32).reshape(-1)), i
    ranges = r.out("frame_ranges", np.float32).view(np.uint32)
    want = np.array([first["range"], second["range"], second["range"]], np.float32).view(np.uint32).reshape(-1)     # the third call wrote nothing back
    assert np.array_equal(ranges, want), (r.out("frame_ranges", np.float32), first["range"], second["range"])
    assert np.array_equal(r.out("frame_counts", np.int32), np.concatenate([first["counts"], second["counts"]]))
    # ---- w[1] == 0: :1072, :1179
    r = shim_driver.run("test_depth_image_shim", tmp_path, arrays, "onelevel")
    assert list(r.out("onelevel_info", np.int32)[:2]) == [0, 0]
    assert np.array_equal(r.out("onelevel_ranges", np.float32), np.full(6, -1, np.float32))
