"""sdso_ingest_frame on the device: raw 8- / 16-bit images in, pyramids out, with the bits sdso_make_pyramid produces from the image the
CPU statement of Undistort::undistort (tests/undistort_ref.py) gives.  The device receives the statement's own remap tables, so every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import helpers
import ingest_cases as Cs
import synth
import undistort_ref as R
from sdso_amd import abi

pytestmark = pytest.mark.gpu
f32 = np.float32

CALIB = 7
SLOTS = (701, 702)      # ingested
WANT = (711, 712)       # sdso_make_pyramid of the statement's image


def _remap(model, size, mode=R.CROP, oc=None):
    _, rx, ry, _ = R.make_remap(model, Cs.pars(model, size), size["wOrg"], size["hOrg"], size["w"], size["h"], mode, oc)
    return rx, ry


def _quirk_remap():
    """A pinhole view shifted 100 rows down: rows below the raw image pass Undistort.cpp:939 (iy < wOrg-1) and would be read out of
    bounds by the reference; the library turns them into "outside"."""
    p = np.array([400.0, 400.0, 319.5, 239.5, 0.0])
    _, rx, ry, _ = R.make_remap(R.PINHOLE, p, 640, 480, 640, 480, R.EXPLICIT, [400.0 / 640, 400.0 / 480, 0.5, 140.0 / 480])
    assert ((ry >= 479) & (rx >= 0)).sum() > 50000
    return rx, ry


HAND_KEPT = {(10, 5): (33.25, -0.25), (10, 6): (34.5, -0.999), (10, 7): (-0.0, 17.5), (10, 8): (638.99, 478.99), (10, 9): (0.0, -0.5)}
HAND_OUTSIDE = {(20, 5): (33.25, -1.0), (20, 6): (33.25, -1.5), (20, 7): (np.nan, 17.5), (20, 8): (33.25, np.nan), (20, 9): (np.inf, 17.5),
                (20, 10): (33.25, np.inf), (20, 11): (33.25, -np.inf), (20, 12): (639.0, 17.5), (20, 13): (33.25, 479.0), (20, 14): (np.nan, np.nan),
                (20, 15): (-np.inf, 17.5), (20, 16): (1e30, 1e30)}


def _hand_made_remap():
    """Entries no Undistort object produces but a caller-owned table may hold, written into a pinhole table at (row, column): rows in
    (-1, 0) truncate to row 0 with a negative weight (all four taps exist, so the entry is kept, as the reference would read it); -1 and
    below, the last row or column and beyond, NaN and the infinities have a tap outside the raw image, or none at all, and give 0."""
    rx, ry = [a.copy() for a in _remap(R.PINHOLE, Cs.VGA)]
    for (r, c), (x, y) in {**HAND_KEPT, **HAND_OUTSIDE}.items():
        rx[r, c], ry[r, c] = f32(x), f32(y)
    return rx, ry


def _check(ctx, size, bits, mode, remap, exposures, factor=1.0, with_G=True, use_exposure=True, seed=11):
    """Ingest len(exposures) images and compare every level of every eye with sdso_make_pyramid of the statement's image."""
    n = len(exposures)
    wOrg, hOrg, w, h = size["wOrg"], size["hOrg"], size["w"], size["h"]
    raws = [Cs.raw_image(wOrg, hOrg, bits, seed + i) for i in range(n)]
    G = Cs.response(bits) if with_G else None
    vinv = Cs.vignette_inv(wOrg, hOrg)
    assert Cs.calib_create(ctx, CALIB, size, remap, bits, G, vinv, mode, use_exposure) == 0, ctx.L.sdso_last_error(ctx.h)
    try:
        ex_out = ctx.ingest_frame(CALIB, SLOTS[:n], raws, exposures, factor)
        ctx.sync()
        safe = R.sanitize_remap(remap[0], remap[1], wOrg, hOrg) if remap is not None else (None, None)
        for i in range(n):
            img, ex = R.undistort(raws[i], safe[0], safe[1], G, vinv, mode, exposures[i], factor, use_exposure)
            assert img.shape == (h, w) and ex_out[i] == ex
            Cs.make_pyramid(ctx, WANT[i], img)
            got, want = Cs.download_pyramid(ctx, SLOTS[i], w, h), Cs.download_pyramid(ctx, WANT[i], w, h)
            assert len(got) == synth.pyramid_levels(w, h) and np.abs(want[0][0][..., 0]).max() > 1.0
            assert want[0][0][..., 0].tobytes() == img.tobytes()
            for lvl, (a, b) in enumerate(zip(got, want)):
                assert a[0].tobytes() == b[0].tobytes(), "eye %d level %d: dI differs in %d values" % (i, lvl, (a[0] != b[0]).sum())
                assert a[1].tobytes() == b[1].tobytes(), "eye %d level %d: absSquaredGrad differs" % (i, lvl)
        return raws
    finally:
        ctx.check(ctx.L.sdso_ingest_calib_release(ctx.h, CALIB))


CASES = {
    # name: (size, bits, photometricCalibration, remap, exposures, factor, with_G, use_exposure)
    "kitti-8bit-mode2": (Cs.KITTI, 8, 2, lambda: _remap(R.RADTAN, Cs.KITTI), (0.011, 0.013), 1.0, True, True),
    "kitti-16bit-mode2": (Cs.KITTI, 16, 2, lambda: _remap(R.EQUIDISTANT, Cs.KITTI), (0.011, 0.013), 1.0, True, True),
    "kitti-8bit-mode1": (Cs.KITTI, 8, 1, lambda: _remap(R.FOV, Cs.KITTI), (0.5, 0.5), 1.0, True, True),
    "vga-16bit-mode1": (Cs.VGA, 16, 1, lambda: _remap(R.KANNALABRANDT, Cs.VGA), (0.5, 0.25), 1.0, True, True),
    "vga-8bit-mode0": (Cs.VGA, 8, 0, lambda: _remap(R.PINHOLE, Cs.VGA), (0.5, 0.5), 0.75, True, True),
    "vga-16bit-mode0": (Cs.VGA, 16, 0, lambda: _remap(R.RADTAN, Cs.VGA), (0.5, 0.5), 1.0 / 256, True, True),
    "no-G": (Cs.KITTI, 8, 2, lambda: _remap(R.RADTAN, Cs.KITTI), (0.011, 0.013), 1.25, False, True),
    "exposure-not-positive": (Cs.VGA, 8, 2, lambda: _remap(R.RADTAN, Cs.VGA), (0.0, 0.02), 0.5, True, True),     # left eye linear, right eye calibrated
    "exposure-negative-16bit": (Cs.VGA, 16, 2, lambda: _remap(R.RADTAN, Cs.VGA), (0.02, -1.0), 0.01, True, True),
    "useExposure-off": (Cs.VGA, 8, 2, lambda: _remap(R.RADTAN, Cs.VGA), (0.02, 0.03), 1.0, True, False),
    "passthrough-8bit": (Cs.VGA, 8, 2, lambda: None, (0.02, 0.03), 1.0, True, True),
    "passthrough-16bit-mode0": (Cs.VGA, 16, 0, lambda: None, (0.02, 0.03), 0.01, True, True),
    "minus-one-entries": (Cs.VGA, 8, 2, lambda: _remap(R.RADTAN, Cs.VGA, R.EXPLICIT, Cs.WIDE_K), (0.02, 0.03), 1.0, True, True),
    "taps-leave-the-image": (Cs.VGA, 8, 1, _quirk_remap, (0.02, 0.03), 1.0, True, True),
    "hand-made-entries": (Cs.VGA, 8, 2, _hand_made_remap, (0.02, 0.03), 1.0, True, True),
    "one-image": (Cs.KITTI, 8, 2, lambda: _remap(R.RADTAN, Cs.KITTI), (0.011,), 1.0, True, True),
    "one-image-16bit": (Cs.VGA, 16, 2, lambda: _remap(R.FOV, Cs.VGA), (0.011,), 1.0, True, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ingest_matches_undistort_then_make_pyramid(gpu_ctx, name):
    size, bits, mode, remap, exposures, factor, with_G, use_exposure = CASES[name]
    rm = remap()
    if name == "minus-one-entries":
        assert (rm[0] < 0).sum() > 10000
    if name == "hand-made-entries":        # the rule itself, stated by hand: what the comparison below feeds the statement
        sx, sy = R.sanitize_remap(rm[0], rm[1], size["wOrg"], size["hOrg"])
        for rc, (x, y) in HAND_KEPT.items():
            assert sx[rc].tobytes() == f32(x).tobytes() and sy[rc].tobytes() == f32(y).tobytes()
        for rc in HAND_OUTSIDE:
            assert sx[rc] == -1 and sy[rc] == -1
        img, _ = R.undistort(Cs.raw_image(size["wOrg"], size["hOrg"], bits, 11), sx, sy, Cs.response(bits), Cs.vignette_inv(size["wOrg"], size["hOrg"]),
                             mode, exposures[0], factor, use_exposure)
        assert all(img[rc] == 0 for rc in HAND_OUTSIDE) and all(img[rc] != 0 for rc in HAND_KEPT)
    _check(gpu_ctx, size, bits, mode, rm, exposures, factor, with_G, use_exposure)


@pytest.mark.parametrize("name", ["kitti-8bit-mode2", "vga-16bit-mode1", "minus-one-entries"])
def test_ingest_with_gamma_weights(gpu_ctx, name):
    """sdso_set_gamma applies to an ingested pyramid as to any other (HessianBlocks.cpp:194-198)."""
    size, bits, mode, remap, exposures, factor, with_G, use_exposure = CASES[name]
    Binv = (255.0 * (np.arange(256) / 255.0) ** 1.6).astype(f32)
    B = np.zeros(256, f32)
    assert gpu_ctx.L.sdso_gamma_from_binv(abi.fp(Binv), abi.fp(B)) == 0
    gpu_ctx.check(gpu_ctx.L.sdso_set_gamma(gpu_ctx.h, abi.fp(B)))
    try:
        _check(gpu_ctx, size, bits, mode, remap(), exposures, factor, with_G, use_exposure)
        w, h = size["w"], size["h"]
        weighted = Cs.download_pyramid(gpu_ctx, SLOTS[0], w, h)[0][1].copy()
    finally:
        gpu_ctx.check(gpu_ctx.L.sdso_set_gamma(gpu_ctx.h, None))
    _check(gpu_ctx, size, bits, mode, remap(), exposures, factor, with_G, use_exposure)
    assert not np.array_equal(weighted, Cs.download_pyramid(gpu_ctx, SLOTS[0], w, h)[0][1])     # the weight did change absSquaredGrad


def test_ingest_does_not_synchronise(gpu_ctx):
    """Two ingests into different slots issued back to back and ONE sdso_ctx_sync give the bits of two synchronised ones; the caller's
    raw buffers are overwritten as soon as each call returns."""
    ctx, size = gpu_ctx, Cs.KITTI
    wOrg, hOrg, w, h = size["wOrg"], size["hOrg"], size["w"], size["h"]
    rm = _remap(R.RADTAN, size)
    G, vinv = Cs.response(8), Cs.vignette_inv(wOrg, hOrg)
    frames = [[Cs.raw_image(wOrg, hOrg, 8, 30 + 2 * f + i) for i in range(2)] for f in range(3)]
    slots = [(721, 722), (723, 724), (725, 726)]
    assert Cs.calib_create(ctx, CALIB, size, rm, 8, G, vinv, 2) == 0
    try:
        # synchronised, one by one
        want = []
        for f in range(3):
            ctx.ingest_frame(CALIB, SLOTS, frames[f], (0.01, 0.02))
            ctx.sync()
            want.append([Cs.download_pyramid(ctx, s, w, h) for s in SLOTS])
        # back to back out of ONE pair of buffers that is overwritten after every call (three calls: the staging takes turns)
        bufs = [np.zeros((hOrg, wOrg), np.uint8) for _ in range(2)]
        ptrs = (C.c_void_p * 2)(*[b.ctypes.data for b in bufs])
        ex = np.array([0.01, 0.02], f32)
        for f in range(3):
            for i in range(2):
                bufs[i][...] = frames[f][i]
            ctx.check(ctx.L.sdso_ingest_frame(ctx.h, CALIB, 2, (C.c_int * 2)(*slots[f]), ptrs, abi.fp(ex), 1.0, None))
            for i in range(2):
                bufs[i][...] = 0xA5
        ctx.sync()
        for f in range(3):
            for i in range(2):
                assert Cs.same_bits(Cs.download_pyramid(ctx, slots[f][i], w, h), want[f][i]), "frame %d eye %d" % (f, i)
        assert not Cs.same_bits(want[0][0], want[1][0])
    finally:
        ctx.check(ctx.L.sdso_ingest_calib_release(ctx.h, CALIB))
        for s in sum(slots, ()):
            ctx.L.sdso_release_pyramid(ctx.h, s)


def test_consumers_see_the_same_pyramid(gpu_ctx):
    """sdso_pixel_select and one sdso_track_calc_res_gs evaluation on an ingested slot equal the same calls on a sdso_make_pyramid slot
    of the same image."""
    ctx, size = gpu_ctx, Cs.VGA
    raws = _check(ctx, size, 8, 2, _remap(R.RADTAN, size), (0.02, 0.03))          # leaves SLOTS (ingested) and WANT (make_pyramid) behind
    w, h = size["w"], size["h"]
    sel = []
    for slot in (SLOTS[0], WANT[0]):
        m = np.zeros((h, w), f32); pot = C.c_int(3); n = C.c_int(0)
        ctx.check(ctx.L.sdso_pixel_select(ctx.h, slot, 1500.0, 1, 1.0, C.byref(pot), abi.fp(m), C.byref(n)))
        sel.append((m, pot.value, n.value))
    assert sel[0][1:] == sel[1][1:] and sel[0][2] > 500 and np.array_equal(sel[0][0], sel[1][0])
    prob = synth.tracker_problem(w=w, h=h, npts=1500, seed=5)
    ctx.set_ref(731, prob["pc"])
    try:
        prm = helpers.track_params(prob)
        ev = abi.TrackEval()
        T = synth.se3_exp(np.array([0.01, -0.005, 0.02, 0.002, -0.001, 0.003]))
        ctx.L.sdso_track_make_eval(C.byref(prm), 0, C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(0.01, 0.5)), 1.0, C.byref(ev))
        out = []
        for slot in (SLOTS[1], WANT[1]):
            npts = len(prob["pc"][0]["u"])
            H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0); mask = np.zeros(npts, np.uint8)
            ctx.check(ctx.L.sdso_track_calc_res_gs(ctx.h, 731, slot, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res), C.byref(nw), abi.bp(mask)))
            out.append((H.tobytes(), b.tobytes(), res.tobytes(), nw.value, mask.tobytes()))
        assert out[0] == out[1] and out[0][3] > 100
    finally:
        ctx.L.sdso_track_release_ref(ctx.h, 731)


def test_end_to_end_with_the_library_tables(gpu_ctx):
    """sdso_undistort_make_remap (RadTan, crop) -> sdso_ingest_calib_create -> sdso_ingest_frame against the statement with ITS tables."""
    size = Cs.KITTI
    rc, K, lx, ly, pt = Cs.lib_make_remap(R.RADTAN, Cs.pars(R.RADTAN, size), size, R.CROP)
    Kr, rx, ry, _ = R.make_remap(R.RADTAN, Cs.pars(R.RADTAN, size), size["wOrg"], size["hOrg"], size["w"], size["h"], R.CROP)
    assert rc == 0 and pt == 0 and K.tobytes() == Kr.tobytes()
    ctx = gpu_ctx
    raws = [Cs.raw_image(size["wOrg"], size["hOrg"], 8, 50 + i) for i in range(2)]
    G, vinv = Cs.response(8), Cs.vignette_inv(size["wOrg"], size["hOrg"])
    assert Cs.calib_create(ctx, CALIB, size, (lx, ly), 8, G, vinv, 2) == 0
    try:
        ctx.ingest_frame(CALIB, SLOTS, raws, (0.01, 0.02))
        ctx.sync()
        for i in range(2):
            img, _ = R.undistort(raws[i], rx, ry, G, vinv, 2, 0.01)
            Cs.make_pyramid(ctx, WANT[i], img)
            assert Cs.same_bits(Cs.download_pyramid(ctx, SLOTS[i], size["w"], size["h"]), Cs.download_pyramid(ctx, WANT[i], size["w"], size["h"]))
    finally:
        ctx.check(ctx.L.sdso_ingest_calib_release(ctx.h, CALIB))


def test_refusals_leave_slots_untouched(gpu_ctx):
    ctx, size = gpu_ctx, Cs.VGA
    wOrg, hOrg, w, h = size["wOrg"], size["hOrg"], size["w"], size["h"]
    L = ctx.L
    raws = [Cs.raw_image(wOrg, hOrg, 8, 60 + i) for i in range(2)]
    rm = _remap(R.PINHOLE, size)
    G, vinv = Cs.response(8), Cs.vignette_inv(wOrg, hOrg)
    # calib_create: bad pixel width, bad mode, passthrough with unequal sizes, one remap array only, mode 2 without a vignette
    assert Cs.calib_create(ctx, CALIB, size, rm, 24, G, vinv, 2) == -1
    assert Cs.calib_create(ctx, CALIB, size, rm, 8, G, vinv, 3) == -1
    assert Cs.calib_create(ctx, CALIB, Cs.KITTI, None, 8, G, vinv, 2) == -1
    assert Cs.calib_create(ctx, CALIB, size, rm, 8, G, None, 2) == -1
    assert L.sdso_ingest_calib_create(ctx.h, CALIB, wOrg, hOrg, w, h, abi.fp(rm[0]), None, 1, None, None, 0, 1) == -1
    ex = np.array([0.01, 0.02], f32)
    ptrs = (C.c_void_p * 2)(*[r.ctypes.data for r in raws])
    slots = (C.c_int * 2)(*SLOTS)
    assert L.sdso_ingest_frame(ctx.h, CALIB, 2, slots, ptrs, abi.fp(ex), 1.0, None) == -1            # no such calibration (yet)
    assert Cs.calib_create(ctx, CALIB, size, rm, 8, G, vinv, 2) == 0
    try:
        ctx.ingest_frame(CALIB, SLOTS, raws, ex)
        ctx.sync()
        before = [Cs.download_pyramid(ctx, s, w, h) for s in SLOTS]
        other = [np.ascontiguousarray(r[::-1]) for r in raws]
        optrs = (C.c_void_p * 2)(*[r.ctypes.data for r in other])
        assert L.sdso_ingest_frame(ctx.h, CALIB + 1, 2, slots, optrs, abi.fp(ex), 1.0, None) == -1   # unknown calib
        assert L.sdso_ingest_frame(ctx.h, CALIB, 0, slots, optrs, abi.fp(ex), 1.0, None) == -1       # n_images outside 1..2
        assert L.sdso_ingest_frame(ctx.h, CALIB, 3, slots, optrs, abi.fp(ex), 1.0, None) == -1
        assert L.sdso_ingest_frame(ctx.h, CALIB, 2, (C.c_int * 2)(SLOTS[0], SLOTS[0]), optrs, abi.fp(ex), 1.0, None) == -1   # a slot named twice
        assert L.sdso_ingest_frame(ctx.h, CALIB, 2, slots, (C.c_void_p * 2)(other[0].ctypes.data, None), abi.fp(ex), 1.0, None) == -1   # a null image
        assert L.sdso_ingest_frame(ctx.h, CALIB, 2, None, optrs, abi.fp(ex), 1.0, None) == -1
        assert L.sdso_ingest_frame(None, CALIB, 2, slots, optrs, abi.fp(ex), 1.0, None) == -4
        ctx.sync()
        for s, b in zip(SLOTS, before):
            assert Cs.same_bits(Cs.download_pyramid(ctx, s, w, h), b)
        # and the calibration still works afterwards
        ctx.ingest_frame(CALIB, SLOTS, other, ex)
        ctx.sync()
        assert not Cs.same_bits(Cs.download_pyramid(ctx, SLOTS[0], w, h), before[0])
    finally:
        ctx.check(L.sdso_ingest_calib_release(ctx.h, CALIB))
    assert L.sdso_ingest_frame(ctx.h, CALIB, 2, slots, ptrs, abi.fp(ex), 1.0, None) == -1            # released


def test_level0_kernel_is_profiled_by_name(gpu_ctx):
    ctx, size = gpu_ctx, Cs.VGA
    raws = [Cs.raw_image(size["wOrg"], size["hOrg"], 8, 70 + i) for i in range(2)]
    assert Cs.calib_create(ctx, CALIB, size, _remap(R.PINHOLE, size), 8, None, None, 0) == 0
    try:
        ctx.check(ctx.L.sdso_prof_reset(ctx.h))
        ctx.check(ctx.L.sdso_prof_enable(ctx.h, 1))
        for _ in range(3):
            ctx.ingest_frame(CALIB, SLOTS, raws, (1.0, 1.0))
        ms, launches = ctx.prof_read("k_ingest_level0")
        assert launches == 3 and 0 < ms < 50                                       # one launch covers both eyes
    finally:
        ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
        ctx.check(ctx.L.sdso_prof_reset(ctx.h))
        ctx.check(ctx.L.sdso_ingest_calib_release(ctx.h, CALIB))
