"""sdso_shim::ImmaturePoints (host/sdso_shim.h) driven by host/test_immature_shim.cpp on stand-in types: makeNewTraces,
traceNewCoarseNonKey and traceNewCoarseKey on the program's objects leave the same set as the C-ABI path from Python, exactly.  The
driver's window is headed by a frame that never had makeNewTraces (the first keyframe of the reference's own call sequence) and is
traced before any host has points: both are empty loops in the reference and must not fail here."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_cases as Cs
import immature_ref as R
import shim_driver
import synth

f32 = np.float32
DENSITY = 600.0


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_immature_shim")


def test_immature_shim_driver_compiles():
    """CPU: the shim's ImmaturePoints class + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_immature_shim")


@pytest.mark.gpu
def test_shim_members_leave_the_set_of_the_abi_path(gpu_ctx, driver, tmp_path):
    ctx, L = gpu_ctx, gpu_ctx.L
    case = Cs.window_case()
    hosts, frames = case["hosts"][:2], case["frames"][:3]
    nh, nfr = len(hosts), len(frames)
    pyrs = [synth.make_pyramid(np.ascontiguousarray(h_["img"][..., 0])) for h_ in hosts]
    levels = len(pyrs[0])
    cal = synth.kitti_calib(Cs.W, Cs.H)
    poses, affs = [], []
    for T, aff in [(h_["T"], (0.0, 0.0)) for h_ in hosts] + [(F["T"], F["aff"]) for F in frames]:
        Ti = synth.se3_inv(T)
        poses.append(np.concatenate([T[0].ravel(), T[1], Ti[0].ravel(), Ti[1]]))
        affs.append([aff[0], aff[1], 1.0])
    slots_h, slots_f = [940 + k for k in range(nh)], [(950 + 2 * k, 951 + 2 * k) for k in range(nfr)]
    ids = [60 + k for k in range(nh)]
    try:
        # ---- the C-ABI path: select + add (NULL map), then the traces with the geometries the driver will dump
        made = []
        pot = C.c_int(3)                     # PixelSelector::currentPotential lives on from keyframe to keyframe
        for k in range(nh):
            ctx.upload_pyramid(slots_h[k], pyrs[k])
            num = C.c_int(0)
            ctx.check(L.sdso_pixel_select(ctx.h, slots_h[k], DENSITY, 1, 1.0, C.byref(pot), None, C.byref(num)))
            ctx.check(L.sdso_imm_add_frame(ctx.h, ids[k], slots_h[k], None, None))
            made.append(num.value)
        n0 = C.c_int(0)
        ctx.check(L.sdso_imm_count(ctx.h, ids[0], C.byref(n0)))
        flags = (np.arange(n0.value) % 5 == 2).astype(np.uint8); flags[-3:] = 1
        arrays = dict(meta=np.array([Cs.W, Cs.H, levels, nh, nfr], np.int32),
                      calib=np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"], cal["baseline"], DENSITY], f32),
                      poses=np.concatenate(poses).astype(np.float64), affs=np.array(affs, np.float64).ravel(), flags=flags)
        for k in range(nh):
            for l in range(levels):
                arrays["host%d_dI%d" % (k, l)] = pyrs[k][l]
        for k, F in enumerate(frames):
            arrays["frame%d_left" % k] = F["left"]; arrays["frame%d_right" % k] = F["right"]
        r = shim_driver.run("test_immature_shim", tmp_path, arrays, mode="run")
        out = r.out

        assert list(out("made", np.int32)) == made
        kk = out("K4Ki", f32)
        assert np.array_equal(kk[:4], case["K4"]) and np.allclose(kk[4:], case["Ki"], rtol=1e-6, atol=1e-9)
        geoms = out("geoms", f32).reshape(nfr, nh, 26)
        for k, F in enumerate(frames):
            ctx.upload_pyramid(slots_f[k][0], [F["left"]]); ctx.upload_pyramid(slots_f[k][1], [F["right"]])
            G = (abi.ImmGeom * nh)()
            for j in range(nh):
                g = geoms[k, j]
                want = F["geom"][j]      # the same products formed by NumPy: equal up to the rounding of a 3-term sum
                for name, lo, hi in (("KRKi", 0, 9), ("Kt", 9, 12), ("aff", 12, 14), ("KRi", 14, 23), ("t", 23, 26)):
                    getattr(G[j], name)[:] = [float(x) for x in g[lo:hi]]
                    assert np.allclose(g[lo:hi], want[name], rtol=1e-5, atol=1e-4), (k, j, name)
                G[j].host_id = ids[j]
            ctx.check(L.sdso_imm_trace(ctx.h, slots_f[k][0], slots_f[k][1] if k + 1 < nfr else -1, nh, G, abi.fp(kk[:4].copy()), abi.fp(kk[4:].copy()),
                                       float(cal["baseline"]), None))
        for k in range(nh):
            got = shim_driver.unpack_points(out("h%d_f" % k, f32), out("h%d_st" % k, np.uint8))
            want = ctx.imm_get(ids[k])
            assert len(want["u"]) > 100 and R.same(got, want) is None, (k, R.same(got, want))
            assert (want["lastTraceStatus"] == R.GOOD).sum() > 10
        ctx.check(L.sdso_imm_remove(ctx.h, ids[0], len(flags), abi.bp(flags)))
        got = shim_driver.unpack_points(out("removed_f", f32), out("removed_st", np.uint8))
        want = ctx.imm_get(ids[0])
        assert len(want["u"]) == n0.value - int(flags.sum()) and R.same(got, want) is None
        assert r.stdout.split() == ["points", str(len(want["u"])), "0"]
    finally:
        for hid in ids:
            L.sdso_imm_release_host(ctx.h, hid)
        for s in slots_h + [x for p in slots_f for x in p]:
            L.sdso_release_pyramid(ctx.h, s)
