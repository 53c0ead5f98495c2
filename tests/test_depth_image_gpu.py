"""sdso_track_keep_depth_map / sdso_track_depth_image / sdso_track_depth_image_dev: CoarseTracker::debugPlotIDepthMap and
debugPlotIDepthMapFloat (CoarseTracker.cpp:1071-1188) on the device, against the NumPy statement of tests/depth_image_ref.py (literal
loops, the scatter included).  Every comparison is for equality of bytes and float bit patterns.

Templates come from sdso_track_make_ref on synth.tracker_problem pyramids; the points are uniform over the whole image, the two-pixel
border included, where the kept map holds un-normalised sums that the reference's sort counts.  The conditions the shapes were chosen for
are asserted on the reference before anything is compared (and, without a GPU, in tests/test_depth_image_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import depth_image_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
FRAME = {"96x64": 901, "322x242": 902, "640x480": 903}
REF_SHAPE, REF_HAND, REF_SEQ, REF_OFF, REF_SET, REF_WIN, REF_WIN_HOST = 90, 91, 92, 93, 94, 95, 96
KEYS = ("u", "v", "idepth", "color")
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    c.keep_depth_map(True)
    for name, slot in FRAME.items():
        c.upload_pyramid(slot, ref.case(name)["pyr"])
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_ref(ctx, slot, frame, pts):
    u, v = np.ascontiguousarray(pts[0], np.int32), np.ascontiguousarray(pts[1], np.int32)
    idp, wgt = np.ascontiguousarray(pts[2], np.float32), np.ascontiguousarray(pts[3], np.float32)
    pcn = np.zeros(8, np.int32)
    ctx.check(ctx.L.sdso_track_make_ref(ctx.h, slot, frame, len(u), abi.ip(u), abi.ip(v), abi.fp(idp), abi.fp(wgt), abi.ip(pcn)))
    return pcn


def get_ref(ctx, slot, levels):
    out = []
    for l in range(levels):
        nn = C.c_int(-1)
        ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), None, None, None, None))
        arrs = [np.zeros(nn.value, np.float32) for _ in KEYS]
        if nn.value:
            ctx.check(ctx.L.sdso_track_get_ref(ctx.h, slot, l, C.byref(nn), *[abi.fp(a) for a in arrs]))
        out.append(dict(zip(KEYS, arrs)))
    return out


def check_call(got, want, m, prev):
    """one sdso_track_depth_image result against debug_plot's: the map, both counts, the image, the range"""
    assert np.array_equal(bits(got["idepth"]), bits(m)), "%d map pixels differ" % (bits(got["idepth"]) != bits(m)).sum()
    assert tuple(got["counts"]) == tuple(want["counts"]), (got["counts"], want["counts"])
    bad = np.nonzero((got["rgb"] != want["rgb"]).any(axis=2))
    assert len(bad[0]) == 0, "%d image pixels differ, the first at (x %d, y %d): %s, want %s" % (
        len(bad[0]), bad[1][0], bad[0][0], got["rgb"][bad[0][0], bad[1][0]], want["rgb"][bad[0][0], bad[1][0]])
    if prev is None:
        assert got["range"] is None
    else:
        assert np.array_equal(bits(got["range"]), bits(want["prev_out"])), (got["range"], want["prev_out"])


def small():
    c = ref.case("96x64")
    return c["w"], c["h"], c["I0"], FRAME["96x64"]


def run_points(ctx, slot, pts, prev=(-1, -1)):
    """template from `pts` on the 96x64 frame, its image on the device and by the reference"""
    w, h, I0, frame = small()
    make_ref(ctx, slot, frame, pts)
    m = ref.level0_map(*pts, I0)
    want = ref.debug_plot(m, I0, None if prev is None else (f32(prev[0]), f32(prev[1])))
    got = ctx.depth_image(slot, frame, w, h, prev)
    check_call(got, want, m, prev)
    return got, want, m


# ------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_shapes(ctx, name):
    c = ref.case(name)
    cond = ref.input_conditions(name)
    print(name, cond)
    if name == "322x242":
        assert cond["outcomes"] == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8] and cond["circles_without_centre"] >= 2000 and cond["border_positive"] >= 200
    if name == "96x64":
        assert cond["levels"] == 2 and cond["border_positive"] >= 50
    if name == "640x480":
        assert cond["positive"] >= 80000
    make_ref(ctx, REF_SHAPE, FRAME[name], c["points"])
    got = ctx.depth_image(REF_SHAPE, FRAME[name], c["w"], c["h"], (-1, -1))
    print("range", got["range"], "counts", got["counts"], "reference", c["plot"]["used"], c["plot"]["counts"])
    check_call(got, c["plot"], c["map"], (-1, -1))
    # the device images of that call hold the same bytes
    p_rgb, p_id, w, h = ctx.depth_image_dev(REF_SHAPE)
    assert (w, h) == (c["w"], c["h"])
    assert np.array_equal(ctx.read_device(p_rgb, w * h * 3), got["rgb"].reshape(-1))
    assert np.array_equal(ctx.read_device(p_id, w * h * 4).view(np.uint32), bits(got["idepth"]).reshape(-1))
    # either image alone
    only_rgb = ctx.depth_image(REF_SHAPE, FRAME[name], c["w"], c["h"], (-1, -1), idepth=False)
    only_id = ctx.depth_image(REF_SHAPE, FRAME[name], c["w"], c["h"], (-1, -1), rgb=False)
    assert np.array_equal(only_rgb["rgb"], got["rgb"]) and np.array_equal(bits(only_id["idepth"]), bits(got["idepth"]))
    assert tuple(only_rgb["counts"]) == tuple(only_id["counts"]) == tuple(got["counts"])


# ------------------------------------------------------------------ hand-built
def test_three_neighbours_draw_a_circle(ctx):
    """points at (x-1, y), (x+1, y), (x, y+1) only: (x, y) stays -1 (no diagonal neighbour of it carries weight) and draws through nid >= 3"""
    x, y = 40, 30
    pts = (np.array([x - 1, x + 1, x]), np.array([y, y, y + 1]), np.array([0.4, 0.8, 1.2], f32), np.ones(3, f32))
    got, want, m = run_points(ctx, REF_HAND, pts)
    assert m[y, x] == -1
    ys, xs = want["sources"]
    k = np.nonzero((ys == y) & (xs == x))[0]
    assert len(k) == 1 and not want["centre_positive"][k[0]]
    assert (~want["centre_positive"]).sum() >= 1 and got["counts"][1] == len(ys)


@pytest.mark.parametrize("step", [(3, 0), (0, 3)], ids=["horizontal", "vertical"])
def test_later_source_overwrites(ctx, step):
    """two qualifying sources three pixels apart: where both rings fall, the later one in raster order shows"""
    x, y = 30, 20
    x2, y2 = x + step[0], y + step[1]
    pts = (np.array([x, x2]), np.array([y, y2]), np.array([0.3, 1.6], f32), np.ones(2, f32))
    got, want, m = run_points(ctx, REF_HAND, pts)
    assert m[y, x] == f32(0.3) and m[y2, x2] == f32(1.6)
    ys, xs = want["sources"]
    k1, k2 = np.nonzero((ys == y) & (xs == x))[0], np.nonzero((ys == y2) & (xs == x2))[0]
    assert len(k1) == 1 and len(k2) == 1 and k1[0] < k2[0]
    # the two colours differ, so an overlap that showed the earlier source would differ from the reference (run_points compared the image)
    span = want["used"][1] - want["used"][0]
    lo, _ = ref.make_jet_3b(np.array([(f32(0.3) - want["used"][0]) / span], f32))
    hi, _ = ref.make_jet_3b(np.array([(f32(1.6) - want["used"][0]) / span], f32))
    assert tuple(lo[0]) != tuple(hi[0])
    # each centre lies on the other's ring, three pixels away, and nothing later in raster order reaches the earlier centre
    assert tuple(got["rgb"][y, x]) == tuple(hi[0])


def test_smoothing_sequence(ctx):
    """(-1, -1) takes the range over; a template whose percentiles jump up by more than 30 % of the span, then down, is followed at
    0.3 * span per call"""
    rs = np.random.RandomState(17)
    base = (rs.randint(4, 92, 300), rs.randint(4, 60, 300), rs.uniform(0.05, 2.0, 300).astype(f32), rs.uniform(0.1, 30.0, 300).astype(f32))
    prev = (f32(-1), f32(-1))
    seen = []
    for scale in (1.0, 6.0, 0.02):
        pts = (base[0], base[1], (base[2] * f32(scale)).astype(f32), base[3])
        got, want, m = run_points(ctx, REF_SEQ, pts, prev)
        seen.append((want["new"], want["used"]))
        print("scale", scale, "new", want["new"], "used", want["used"], "device", got["range"])
        prev = got["range"]
    (n0, u0), (n1, u1), (n2, u2) = seen
    assert u0 == n0
    step1, step2 = f32(0.3) * (u0[1] - u0[0]), f32(0.3) * (u1[1] - u1[0])
    assert n1[0] > u0[0] + step1 and n1[1] > u0[1] + step1 and u0[0] < u1[0] < n1[0] and u0[1] < u1[1] < n1[1]       # clamped on the way up
    assert n2[0] < u1[0] - step2 and n2[1] < u1[1] - step2 and n2[0] < u2[0] < u1[0] and n2[1] < u2[1] < u1[1]       # and on the way down


def test_null_range_pointers(ctx):
    """both NULL: the new range is used, nothing is written back; one NULL: SDSO_ERR_ARG"""
    w, h, I0, frame = small()
    got, want, m = run_points(ctx, REF_HAND, ref.case("96x64")["points"], prev=None)
    assert want["used"] == want["new"]
    one = np.array([0.25], f32)
    for a, b in ((abi.fp(one), None), (None, abi.fp(one))):
        rgb = np.full((h, w, 3), 77, np.uint8)
        assert ctx.L.sdso_track_depth_image(ctx.h, REF_HAND, frame, a, b, abi.bp(rgb), None, None) == ERR_ARG
        assert one[0] == f32(0.25) and (rgb == 77).all()


def test_all_depths_equal(ctx):
    """maxID == minID: id = 0/0 is NaN (white), a smaller / larger depth gives -inf / +inf, which the two clamps take"""
    rs = np.random.RandomState(5)
    cells = rs.permutation(((96 - 12) // 2) * ((64 - 12) // 2))[:400]          # distinct pixels, two apart, away from the border
    u, v = 6 + 2 * (cells % 42), 6 + 2 * (cells // 42)
    idp = np.full(400, 0.5, f32)
    idp[0], idp[1] = 0.25, 1.0
    got, want, m = run_points(ctx, REF_HAND, (u, v, idp, np.ones(400, f32)))
    assert want["used"][0] == want["used"][1] == f32(0.5)
    assert {9, -1, 8} <= set(want["case"].tolist())
    assert (got["rgb"] == 255).all(axis=2).any()


def test_empty_template(ctx):
    w, h, I0, frame = small()
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, f32), np.zeros(0, f32))
    got, want, m = run_points(ctx, REF_HAND, none, prev=(0.3, 0.9))
    assert tuple(got["counts"]) == (0, 0) and got["range"] == (f32(0.3), f32(0.9))
    assert np.array_equal(got["rgb"], np.repeat(ref.background(I0)[:, :, None], 3, axis=2))
    assert (got["idepth"][2:-2, 2:-2] == -1).all() and (got["idepth"] > 0).sum() == 0


# ------------------------------------------------------------------ refusals, the switch
def test_refusals_and_switch(ctx):
    w, h, I0, frame = small()
    pts = ref.case("96x64")["points"]
    make_ref(ctx, REF_HAND, frame, pts)
    with_map = get_ref(ctx, REF_HAND, 2)
    # a frame of another size, unknown slots
    assert ctx.depth_image_raw(REF_HAND, FRAME["322x242"], w, h, (-1, -1))[0] == ERR_ARG
    assert ctx.depth_image_raw(REF_HAND, 4242, w, h, (-1, -1))[0] == ERR_ARG
    assert ctx.depth_image_raw(4242, frame, w, h, (-1, -1))[0] == ERR_ARG
    # a template sdso_track_set_ref installed has no map — on a fresh slot, and over a template that had one
    for slot in (REF_SET, REF_HAND):
        ctx.set_ref(slot, with_map)
        rc, d = ctx.depth_image_raw(slot, frame, w, h, (-1, -1))
        assert rc == ERR_STATE and (d["rgb"] == 77).all() and (d["idepth"] == -7).all() and (d["counts"] == -1).all()
    # the switch off: no map, and the same template
    ctx.keep_depth_map(False)
    try:
        make_ref(ctx, REF_OFF, frame, pts)
        assert ctx.depth_image_raw(REF_OFF, frame, w, h, (-1, -1))[0] == ERR_STATE
        without = get_ref(ctx, REF_OFF, 2)
        p = C.c_void_p()
        ww, hh = C.c_int(0), C.c_int(0)
        assert ctx.L.sdso_track_depth_image_dev(ctx.h, REF_OFF, C.byref(p), C.byref(p), C.byref(ww), C.byref(hh)) == ERR_STATE
    finally:
        ctx.keep_depth_map(True)
    for a, b in zip(with_map, without):
        assert len(a["u"]) == len(b["u"]) > 0
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    # switched on again, the slot built while it was off gets its map with its next template
    make_ref(ctx, REF_OFF, frame, pts)
    check_call(ctx.depth_image(REF_OFF, frame, w, h, (-1, -1)), ref.case("96x64")["plot"], ref.case("96x64")["map"], (-1, -1))
    ctx.check(ctx.L.sdso_track_release_ref(ctx.h, REF_OFF))
    assert ctx.depth_image_raw(REF_OFF, frame, w, h, (-1, -1))[0] == ERR_ARG


# ------------------------------------------------------------------ through sdso_track_make_ref_from_window
def test_from_window_keeps_the_same_map(ctx):
    import tracking_ref_window_cases as TC
    case = TC.make_case(nf=4, pts_per_kf=200, seed=3101)
    up = TC.upload(ctx, case, 77, 940)
    TC.optimize(ctx, up["wid"], 3)
    d, pcn, _ = TC.window_route(ctx, up, REF_WIN)
    assert len(d["u"]) > 100
    w, h = case["w"], case["h"]
    a = ctx.depth_image(REF_WIN, up["left"], w, h, (-1, -1))
    make_ref(ctx, REF_WIN_HOST, up["left"], (d["u"], d["v"], d["new_idepth"], d["weight"]))
    b = ctx.depth_image(REF_WIN_HOST, up["left"], w, h, (-1, -1))
    assert np.array_equal(bits(a["idepth"]), bits(b["idepth"])) and (a["idepth"] > 0).sum() > 100
    assert np.array_equal(a["rgb"], b["rgb"]) and tuple(a["counts"]) == tuple(b["counts"]) and a["range"] == b["range"]
    I0 = np.ascontiguousarray(case["pyrs"][-1][0][..., 0])
    m = ref.level0_map(d["u"], d["v"], d["new_idepth"], d["weight"], I0)
    check_call(a, ref.debug_plot(m, I0, (f32(-1), f32(-1))), m, (-1, -1))
    ctx.check(ctx.L.sdso_ba_release_window(ctx.h, up["wid"]))
