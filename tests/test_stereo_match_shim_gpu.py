"""sdso_shim::ImmaturePoints::stereoMatch (host/sdso_shim.h) driven by host/test_stereo_match_shim.cpp on stand-in types: makeNewTraces,
stereoMatch and release on the program's objects give the idepth map and the counter of the C-ABI path from Python, exactly."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_cases as Cs
import shim_driver
import stereo_match_cases as Ms
import stereo_match_ref as M
import synth

f32 = np.float32
DENSITY = 600.0
SLOT_L, SLOT_R, HOST_ID = 970, 971, 80


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_stereo_match_shim")


def test_stereo_match_shim_driver_compiles():
    """CPU: the shim's stereoMatch member + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_stereo_match_shim")


@pytest.mark.gpu
def test_shim_stereo_match_gives_the_map_of_the_abi_path(gpu_ctx, driver, tmp_path):
    ctx, L = gpu_ctx, gpu_ctx.L
    c = Ms.pair()
    pyr = synth.make_pyramid(np.ascontiguousarray(c["left"][..., 0]))
    cal = synth.kitti_calib(Cs.W, Cs.H)
    try:
        # ---- the C-ABI path: select + add (NULL map) + sdso_imm_stereo_match with the dense map
        ctx.upload_pyramid(SLOT_L, pyr); ctx.upload_pyramid(SLOT_R, [c["right"]])
        pot = C.c_int(3); num = C.c_int(0)
        ctx.check(L.sdso_pixel_select(ctx.h, SLOT_L, DENSITY, 1, 1.0, C.byref(pot), None, C.byref(num)))
        ctx.check(L.sdso_imm_add_frame(ctx.h, HOST_ID, SLOT_L, None, None))
        want = ctx.imm_stereo_match(HOST_ID, SLOT_L, SLOT_R, c["K4"], c["baseline"], map_wh=(Cs.W, Cs.H))
        n = int(want["counts"][M.C_WALKED])
        assert n > 300 and want["counts"][M.C_ACCEPTED] > 100

        arrays = dict(meta=np.array([Cs.W, Cs.H, len(pyr)], np.int32),
                      calib=np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"], cal["baseline"], DENSITY], f32), right=c["right"])
        for l, p in enumerate(pyr):
            arrays["left_dI%d" % l] = p
        r = shim_driver.run("test_stereo_match_shim", tmp_path, arrays, mode="run")
        got = r.out("map", f32).reshape(Cs.H, Cs.W, 3)
        assert got.tobytes() == want["map"].tobytes()
        counter = int(r.out("counter", np.int32)[0])
        assert counter == want["counts"][M.C_ACCEPTED] == (got[..., 0] != 0).sum()
        assert r.stdout.split() == ["matches", str(counter), "points", str(n), "0"]     # the group is gone after release
    finally:
        L.sdso_imm_release_host(ctx.h, HOST_ID)
        for s in (SLOT_L, SLOT_R):
            L.sdso_release_pyramid(ctx.h, s)
