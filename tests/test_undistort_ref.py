"""CPU: the NumPy statement of Undistort (tests/undistort_ref.py) is consistent with itself, and sdso_undistort_make_remap — host-only code
of the library — agrees with it: bit for bit where no transcendental call is involved, within a measured bound where one is."""
import numpy as np
import pytest

import ingest_cases as Cs
import undistort_ref as R
from sdso_amd import abi

f32, f64 = np.float32, np.float64

# profiles/ingest_remap_ulp.txt (tools/ingest_remap_ulp.py): the largest difference between the statement evaluated with float32
# transcendentals and with float64 ones rounded to float32, over every case below, is 0.000244140625 pixels (2 ulp of a coordinate
# beyond 1024); a libm may differ from NumPy by as much.  The library is allowed four times that, for K and for the remap alike.
REMAP_BOUND = 4 * 0.000244140625
FLAG_CAP = 1e-3          # validity flags that may differ next to a threshold of Undistort.cpp:939, as a share of a case's pixels

EXACT = (R.PINHOLE, R.RADTAN)
CASES = Cs.remap_cases()


def _near_threshold(ix, iy, wOrg, bound):
    """The statement's coordinate lies within `bound` of a threshold of :939: 0 and wOrg-1 for ix, 0 and wOrg-1 (sic) for iy."""
    t = f64(wOrg - 1)
    ix, iy = ix.astype(f64), iy.astype(f64)
    with np.errstate(invalid="ignore"):
        return (np.abs(ix) <= bound) | (np.abs(ix - t) <= bound) | (np.abs(iy) <= bound) | (np.abs(iy - t) <= bound)


# ------------------------------------------------------------------ the statement against itself
def test_passthrough_is_the_photometric_image():
    s = Cs.VGA
    raw = Cs.raw_image(s["wOrg"], s["hOrg"], 8, 1)
    G, vinv = Cs.response(8), Cs.vignette_inv(s["wOrg"], s["hOrg"])
    for mode in (0, 1, 2):
        img, ex = R.undistort(raw, None, None, G, vinv, mode, 0.02, factor=1.0)
        want, _ = R.process_frame(raw, G, vinv, mode, 0.02, 1.0)
        assert img.tobytes() == want.tobytes() and ex == f32(0.02)
    # `none` is the only mode that sets passthrough, and it wants equal sizes (:882-895)
    K, _, _, pt = R.make_remap(R.PINHOLE, Cs.pars(R.PINHOLE, s), s["wOrg"], s["hOrg"], s["w"], s["h"], R.NONE)
    assert pt and np.array_equal(K, [0.58 * 640, 0.77 * 480, 0.5012 * 640 - 0.5, 0.4987 * 480 - 0.5])


def test_identity_pinhole_remap_reproduces_interior_pixels():
    s = Cs.VGA
    p = np.array([400.0, 400.0, 319.5, 239.5, 0.0])
    oc = [400.0 / 640, 400.0 / 480, 320.0 / 640, 240.0 / 480]                  # K(0,2) = 0.5 * 640 - 0.5 = 319.5: the same intrinsics
    K, rx, ry, pt = R.make_remap(R.PINHOLE, p, 640, 480, 640, 480, R.EXPLICIT, oc)
    assert not pt and np.array_equal(K, [400.0, 400.0, 319.5, 239.5])
    raw = Cs.raw_image(640, 480, 8, 2)
    with pytest.raises(R.UndistortError):                                      # the last row passes :939 (479 < wOrg-1) and reads past the image
        R.undistort(raw, rx, ry, None, None, 0, 1.0, factor=1.0)
    sx, sy = R.sanitize_remap(rx, ry, 640, 480)
    img, _ = R.undistort(raw, sx, sy, None, None, 0, 1.0, factor=1.0)
    assert (sx[479] == -1).all() and (img[479] == 0).all() and np.array_equal(sx[:479], rx[:479])
    gx, gy = np.meshgrid(np.arange(640), np.arange(480))
    inner = (gx >= 1) & (gx <= 638) & (gy >= 1) & (gy <= 478)
    assert np.abs(rx - gx)[inner].max() <= 1e-4 and np.abs(ry - gy)[inner].max() <= 1e-4
    assert np.abs(img - raw.astype(f32))[inner].max() <= 255 * 4e-4           # the blend of a pixel with weights off by <= 1e-4 each way


def test_photometric_modes_and_exposure_rule():
    s = Cs.VGA
    raw = Cs.raw_image(s["wOrg"], s["hOrg"], 16, 3)
    G, vinv = Cs.response(16), Cs.vignette_inv(s["wOrg"], s["hOrg"])
    lin = (f32(0.25) * raw.astype(f32)).astype(f32)
    g = G[raw]
    for mode, want in ((0, lin), (1, g), (2, (g * vinv).astype(f32))):
        img, ex = R.process_frame(raw, G, vinv, mode, 0.5, 0.25)
        assert img.tobytes() == want.tobytes() and ex == f32(0.5)
    for G_, exposure in ((None, 0.5), (G, 0.0), (G, -1.0)):                     # !valid, exposure_time <= 0 (:231)
        img, ex = R.process_frame(raw, G_, vinv, 2, exposure, 0.25)
        assert img.tobytes() == lin.tobytes() and ex == f32(exposure)
    assert R.process_frame(raw, G, vinv, 2, 0.5, 0.25, use_exposure=False)[1] == f32(1)     # :258-259
    assert R.process_frame(raw, G, vinv, 2, 0.5, 0.25, use_exposure=False)[0].tobytes() == (g * vinv).astype(f32).tobytes()


def test_remap_quirks_are_kept():
    """:937 writes ix when iy == hOrg-1, and :939 compares iy with wOrg-1: with hOrg < wOrg an entry below the image stays "valid"."""
    s = Cs.VGA
    p = np.array([400.0, 400.0, 319.5, 239.5, 0.0])
    oc = [400.0 / 640, 400.0 / 480, 320.0 / 640, (240.0 - 100.0) / 480]       # shifts the view 100 rows down: y runs to 579 > hOrg-1
    _, rx, ry, _ = R.make_remap(R.PINHOLE, p, 640, 480, 640, 480, R.EXPLICIT, oc)
    below = (ry >= 479) & (rx >= 0)
    assert below.sum() > 50000 and ry.max() > 570                              # passed :939 although outside the raw image
    sx, sy = R.sanitize_remap(rx, ry, 640, 480)
    assert (sx[below] == -1).all() and (sy[below] == -1).all() and np.array_equal(sx[~below], rx[~below]) and np.array_equal(sy[~below], ry[~below])
    row = np.nonzero((ry == 479).any(axis=1))[0]                               # the iy == hOrg-1 row: ix overwritten with hOrg-1.001
    assert len(row) == 1 and (rx[row[0]] == f32(480 - 1.001)).all()


def test_statement_evaluations_agree_within_the_cap():
    """The cases are chosen so that the two evaluations of the statement (float32 / float64 transcendentals) already agree within the
    bound and differ in fewer validity flags than the cap; the crops have no -1 entry."""
    for name, model, s, mode, oc in CASES:
        a = R.make_remap(model, Cs.pars(model, s), s["wOrg"], s["hOrg"], s["w"], s["h"], mode, oc, "f32", True)
        b = R.make_remap(model, Cs.pars(model, s), s["wOrg"], s["hOrg"], s["w"], s["h"], mode, oc, "f64", True)
        both = (a[1] >= 0) & (b[1] >= 0)
        d = max(np.abs(a[1] - b[1])[both].max(), np.abs(a[2] - b[2])[both].max(), np.abs(a[0] - b[0]).max())
        flags = (a[1] < 0) != (b[1] < 0)
        print("%s: statement f32 vs f64: max diff %.6g, %d flags of %d" % (name, d, flags.sum(), flags.size))
        assert d <= REMAP_BOUND / 4, name
        assert flags.sum() <= FLAG_CAP * flags.size, name
        assert not (flags & ~_near_threshold(a[4], a[5], s["wOrg"], REMAP_BOUND)).any(), name
        if mode == R.CROP:
            assert (a[1] >= 0).all() and (b[1] >= 0).all(), name
        else:
            assert (a[1] < 0).sum() > 10000, name                              # the wide K does produce a border of -1 entries


# ------------------------------------------------------------------ the library against the statement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_make_remap_matches_the_statement(case):
    name, model, s, mode, oc = case
    p = Cs.pars(model, s)
    K, rx, ry, pt, ix, iy = R.make_remap(model, p, s["wOrg"], s["hOrg"], s["w"], s["h"], mode, oc, "f32", True)
    rc, Kl, lx, ly, ptl = Cs.lib_make_remap(model, p, s, mode, oc)
    assert rc == 0 and ptl == int(pt) == 0
    if model in EXACT:                                                         # no transcendental call: every bit
        assert Kl.tobytes() == K.tobytes() and lx.tobytes() == rx.tobytes() and ly.tobytes() == ry.tobytes()
        return
    dK = np.abs(Kl - K).max()
    flags = (lx < 0) != (rx < 0)
    both = (lx >= 0) & (rx >= 0)
    d = max(np.abs(lx - rx)[both].max(), np.abs(ly - ry)[both].max())
    print("%s: library vs statement: K %.6g, remap %.6g pixels, %d flags of %d" % (name, dK, d, flags.sum(), flags.size))
    assert dK <= REMAP_BOUND and d <= REMAP_BOUND
    assert ((lx < 0) == (ly < 0)).all()
    assert not (flags & ~_near_threshold(ix, iy, s["wOrg"], REMAP_BOUND)).any()
    assert flags.sum() <= FLAG_CAP * flags.size
    if mode == R.CROP:
        assert (lx >= 0).all() and (rx >= 0).all()


def test_make_remap_none_mode_and_relative_format():
    s = Cs.VGA
    for model in (R.PINHOLE, R.RADTAN):
        p = Cs.pars(model, s)                                                  # relative format: rescaled by :793-809 on both sides
        K, rx, ry, pt = R.make_remap(model, p, 640, 480, 640, 480, R.NONE)
        rc, Kl, lx, ly, ptl = Cs.lib_make_remap(model, p, s, R.NONE)
        assert rc == 0 and ptl == 1 and pt
        assert Kl.tobytes() == K.tobytes() and lx.tobytes() == rx.tobytes() and ly.tobytes() == ry.tobytes()


def test_make_remap_refusals():
    s = Cs.KITTI
    p = Cs.pars(R.RADTAN, s)
    # makeOptimalK_full asserts in the reference (:711-714)
    assert Cs.lib_make_remap(R.RADTAN, p, s, R.FULL)[0] == -1
    with pytest.raises(R.UndistortError):
        R.make_remap(R.RADTAN, p, s["wOrg"], s["hOrg"], s["w"], s["h"], R.FULL)
    # `none` with unequal sizes (:884-888)
    assert Cs.lib_make_remap(R.RADTAN, p, s, R.NONE)[0] == -1
    with pytest.raises(R.UndistortError):
        R.make_remap(R.RADTAN, p, s["wOrg"], s["hOrg"], s["w"], s["h"], R.NONE)
    # a principal point so far right that the image lies beyond the +-5 scan of :599-611: the window stays the single point (cx, cy),
    # which is outside, and 500 shrink steps later the crop gives up (:698-701)
    bad = np.array([718.856, 718.856, 5000.0, 185.0, 0.0])
    assert Cs.lib_make_remap(R.PINHOLE, bad, s, R.CROP)[0] == -1
    with pytest.raises(R.UndistortError):
        R.make_remap(R.PINHOLE, bad, s["wOrg"], s["hOrg"], s["w"], s["h"], R.CROP)
    # and plain bad arguments
    assert Cs.lib_make_remap(7, p, s, R.CROP)[0] == -1
    assert Cs.lib_make_remap(R.RADTAN, p, s, R.EXPLICIT, None)[0] == -1
