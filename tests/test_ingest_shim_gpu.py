"""sdso_shim::Undistort (host/sdso_shim.h) driven by host/test_ingest_shim.cpp on stand-in types: what the program's objects ingest
equals the C-ABI path from Python and the CPU statement on the same inputs, exactly."""

import numpy as np
import pytest

import ingest_cases as Cs
import shim_driver
import synth
import undistort_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_ingest_shim")


def test_ingest_shim_driver_compiles():
    """CPU: the shim's Undistort class + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_ingest_shim")


@pytest.mark.gpu
@pytest.mark.parametrize("bits,size,model", [(8, Cs.KITTI, R.RADTAN), (16, Cs.VGA, R.PINHOLE)])
def test_shim_undistort_ingests_like_the_abi(gpu_ctx, driver, tmp_path, bits, size, model):
    wOrg, hOrg, w, h = size["wOrg"], size["hOrg"], size["w"], size["h"]
    raws = [Cs.raw_image(wOrg, hOrg, bits, 80 + i) for i in range(2)]
    G, vinv = Cs.response(bits), Cs.vignette_inv(wOrg, hOrg)
    exposure = np.array([0.011, 0.013], f32)
    p = Cs.pars(model, size)
    arrays = dict(meta=np.array([wOrg, hOrg, w, h, bits, model, R.CROP, 2, 1], np.int32), pars=np.concatenate([p, np.zeros(8 - len(p))]),
                  out_calib=np.zeros(4, f32), exposure=exposure, G=G, vinv=vinv, raw0=raws[0], raw1=raws[1])
    r = shim_driver.run("test_ingest_shim", tmp_path, arrays, mode="run")
    levels, out = int(r.stdout.split()[1]), r.out
    assert levels == synth.pyramid_levels(w, h)
    # geometry: Pinhole and RadTan have no transcendental call, the tables equal the statement's bit for bit
    K, rx, ry, _ = R.make_remap(model, p, wOrg, hOrg, w, h, R.CROP)
    Ks = out("K", np.float64).reshape(3, 3)
    assert np.array_equal([Ks[0, 0], Ks[1, 1], Ks[0, 2], Ks[1, 2]], K) and Ks[2, 2] == 1 and Ks[0, 1] == 0
    assert out("remapX", f32).tobytes() == rx.tobytes() and out("remapY", f32).tobytes() == ry.tobytes()
    assert np.array_equal(out("exposure", f32), [exposure[0], exposure[1], exposure[0], exposure[1]])
    # the same pair through the C-ABI from here, and sdso_make_pyramid of the statement's image
    assert Cs.calib_create(gpu_ctx, 9, size, (rx, ry), bits, G, vinv, 2) == 0
    try:
        gpu_ctx.ingest_frame(9, (741, 742), raws, exposure)
        gpu_ctx.sync()
        for i in range(2):
            abi_pyr = Cs.download_pyramid(gpu_ctx, 741 + i, w, h)
            img, _ = R.undistort(raws[i], rx, ry, G, vinv, 2, exposure[i])
            Cs.make_pyramid(gpu_ctx, 743, img)
            assert Cs.same_bits(abi_pyr, Cs.download_pyramid(gpu_ctx, 743, w, h))
            for tag in ("a%d" % i, "b%d" % i):        # object A: the stereo call; object B (caller-owned tables): one image per call
                for lvl in range(levels):
                    assert out("%s_dI%d" % (tag, lvl), f32).tobytes() == abi_pyr[lvl][0].tobytes(), (tag, lvl)
                    assert out("%s_ag%d" % (tag, lvl), f32).tobytes() == abi_pyr[lvl][1].tobytes(), (tag, lvl)
    finally:
        gpu_ctx.check(gpu_ctx.L.sdso_ingest_calib_release(gpu_ctx.h, 9))
        for s in (741, 742, 743):
            gpu_ctx.L.sdso_release_pyramid(gpu_ctx.h, s)
