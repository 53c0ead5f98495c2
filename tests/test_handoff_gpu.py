"""Frames and tracking templates handed between contexts, device to device (sdso_pyramid_export / _import, sdso_track_export_ref /
_import_ref, csrc/share.h + share.hip): two (or three) abi.Context(0) in one process.  The feature computes nothing, so every comparison
is by bit pattern: what the importer reads is what the builder reads; an exported block is frozen (a later build into a slot that views
it goes to fresh buffers, on either side); a block outlives its source slot and ctx; what a ctx derives from a pyramid or keeps next to a
template stays that ctx's own; a slot nobody exported keeps its buffers across rebuilds.

320 x 240; the windows of tests/tracking_ref_window_cases.py (4 keyframes x 200 points, 8 x 60), synth images, ingest_cases raw pairs."""
import ctypes as C

import numpy as np
import pytest

import helpers
import ingest_cases as Cs
from sdso_amd import abi
import synth
import tracking_ref_window_cases as TC

pytestmark = pytest.mark.gpu

W, H = 320, 240
ERR_ARG, ERR_STATE = -1, -4
PYR, TPL = 0, 1
SHAPES = {"nf4": dict(nf=4, pts_per_kf=200, seed=3101), "nf8": dict(nf=8, pts_per_kf=60, seed=3102)}
WIN = {"nf4": 61, "nf8": 62}
SLOT0 = {"nf4": 600, "nf8": 620}
REF_A = 65           # the template A builds and exports
REF_B = 31           # where B views it
REF_OWN = {"nf4": 66, "nf8": 67}   # A's own copies of the two templates, never exported


@pytest.fixture(scope="module")
def A():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def B():
    c = abi.Context(0)
    yield c
    c.close()


def image(seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return (120 + 60 * np.sin(x / 11.0 + seed) * np.cos(y / 7.0) + 25 * np.sin((x + 3 * y) / 4.0) + 4 * rs.normal(0, 1, (H, W))).astype(np.float32)


@pytest.fixture(scope="module")
def images(A):
    """two images and the pyramids sdso_make_pyramid builds of them (slots 501 / 502 of A, never exported; downloaded once)"""
    out = {}
    for k, (seed, slot) in {"one": (5, 501), "two": (6, 502)}.items():
        img = image(seed)
        Cs.make_pyramid(A, slot, img)
        out[k] = dict(img=img, pyr=Cs.download_pyramid(A, slot, W, H))
    assert not Cs.same_bits(out["one"]["pyr"], out["two"]["pyr"]) and len(out["one"]["pyr"]) == 3
    return out


@pytest.fixture(scope="module")
def windows(A):
    """per shape: the case, its upload on A, the post-state after 3 iterations, and A's own template of it with its levels"""
    out = {}
    for name, spec in SHAPES.items():
        case = TC.make_case(**spec)
        up = TC.upload(A, case, WIN[name], SLOT0[name])
        TC.optimize(A, up["wid"], 3)
        post = TC.post_state(A, case, up["wid"], projections=False)
        TC.window_route(A, up, REF_OWN[name])
        out[name] = dict(case=case, up=up, post=post, levels=TC.get_ref(A, REF_OWN[name], case["levels"]))
    assert not same_levels(out["nf4"]["levels"], out["nf8"]["levels"])
    assert all(len(a["u"]) > len(b["u"]) > 0 for a, b in zip(out["nf4"]["levels"], out["nf8"]["levels"]))   # nf8 fits nf4's buffers
    return out


def same_levels(a, b):
    return len(a) == len(b) and all(len(x["u"]) == len(y["u"]) and all(np.array_equal(TC.bits(x[k]), TC.bits(y[k])) for k in TC.KEYS) for x, y in zip(a, b))


def down(ctx, slot):
    return Cs.download_pyramid(ctx, slot, W, H)


def test_pyramid(A, B, images):
    Cs.make_pyramid(A, 510, images["one"]["img"])
    h = A.export_pyramid(510)
    assert h.info() == (PYR, 0, 2)
    B.import_pyramid(41, h)                         # another slot number than the source's
    assert h.info() == (PYR, 0, 3)                  # A's slot, the handle, B's slot
    assert Cs.same_bits(down(A, 510), images["one"]["pyr"]) and Cs.same_bits(down(B, 41), images["one"]["pyr"])
    assert A.slot_buffers(PYR, 510) == B.slot_buffers(PYR, 41) and B.slot_buffers(PYR, 41)[1]
    probe = B.export_pyramid(41)                    # (an importer may pass the block on; here: a second handle to read the count through)
    assert probe.info()[2] == 4
    h.release()
    assert probe.info()[2] - 1 == 2                 # without the probe itself: the two slots
    B.check(B.L.sdso_release_pyramid(B.h, 41))
    assert probe.info()[2] == 2 and Cs.same_bits(down(A, 510), images["one"]["pyr"])
    probe.release()
    A.check(A.L.sdso_release_pyramid(A.h, 510))


def test_in_flight(A, B):
    """sdso_ingest_frame only enqueues: export and import follow with no synchronisation in between"""
    size = dict(wOrg=W, hOrg=H, w=W, h=H)
    raws = [Cs.raw_image(W, H, 8, 21 + i) for i in range(2)]
    assert Cs.calib_create(A, 7, size, None, 8, Cs.response(8), Cs.vignette_inv(W, H), 2) == 0, A.L.sdso_last_error(A.h)
    try:
        A.ingest_frame(7, (520, 521), raws, (0.01, 0.02))
        hs = [A.export_pyramid(s) for s in (520, 521)]
        for h, s in zip(hs, (43, 44)):
            B.import_pyramid(s, h)
        got = [down(B, s) for s in (43, 44)]
        A.sync()
        want = [down(A, s) for s in (520, 521)]
        for g, w in zip(got, want):
            assert Cs.same_bits(g, w) and np.abs(w[0][0][..., 0]).max() > 1.0
        assert not Cs.same_bits(want[0], want[1])
        for h in hs:
            h.release()
    finally:
        A.check(A.L.sdso_ingest_calib_release(A.h, 7))
    for s in (520, 521):
        A.check(A.L.sdso_release_pyramid(A.h, s))
    for s in (43, 44):
        B.check(B.L.sdso_release_pyramid(B.h, s))


def test_frozen_both_directions(A, B, images):
    one, two = images["one"], images["two"]
    Cs.make_pyramid(A, 530, one["img"])
    h = A.export_pyramid(530)
    B.import_pyramid(45, h)
    before = A.slot_buffers(PYR, 530)[0]
    Cs.make_pyramid(A, 530, two["img"])                      # same size, same slot: the in-place branch of alloc_pyramid
    after, view = A.slot_buffers(PYR, 530)
    assert not view and not set(before[:3]) & set(after[:3])
    assert Cs.same_bits(down(B, 45), one["pyr"]) and Cs.same_bits(down(A, 530), two["pyr"])
    B.upload_pyramid(45, [lv[0] for lv in two["pyr"]])       # the importer writes into its slot
    assert Cs.same_bits(down(B, 45), two["pyr"]) and not B.slot_buffers(PYR, 45)[1]
    A.import_pyramid(531, h)                                 # the source ctx under another slot
    B.import_pyramid(46, h)                                  # a third import
    assert h.info()[2] == 3
    assert Cs.same_bits(down(A, 531), one["pyr"]) and Cs.same_bits(down(B, 46), one["pyr"])
    assert Cs.same_bits(down(A, 530), two["pyr"])
    h.release()
    for c, s in ((A, 530), (A, 531), (B, 45), (B, 46)):
        c.check(c.L.sdso_release_pyramid(c.h, s))


def test_lifetime(B, images):
    A2 = abi.Context(0)
    try:
        Cs.make_pyramid(A2, 5, images["one"]["img"])
        h1, h2 = A2.export_pyramid(5), A2.export_pyramid(5)
        B.import_pyramid(47, h1)
        A2.check(A2.L.sdso_release_pyramid(A2.h, 5))
    finally:
        A2.close()
    assert Cs.same_bits(down(B, 47), images["one"]["pyr"])
    B.import_pyramid(48, h2)                                 # exported before A2 was closed, imported afterwards
    assert Cs.same_bits(down(B, 48), images["one"]["pyr"])
    h1.release(); h2.release()
    B.check(B.L.sdso_release_pyramid(B.h, 47))
    h3 = B.export_pyramid(48)
    assert h3.info() == (PYR, 0, 2)
    h3.release()
    B.check(B.L.sdso_release_pyramid(B.h, 48))               # the last holder frees it


def _trace(ctx, pr, left, right):
    n = len(pr["u"])
    c, w, g, e = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, left, n, abi.fp(pr["u"]), abi.fp(pr["v"]), abi.fp(c), abi.fp(w), abi.fp(g), abi.fp(e)))
    P, d = abi.make_trace_points(n, pr["u"], pr["v"], c, w, g, e)
    st = np.zeros(n, np.uint8)
    K = np.array(pr["K"], np.float32)
    ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, right, abi.fp(K), float(pr["calib"]["baseline"]), 1, C.byref(P), abi.bp(st)))
    return [c, e, st] + [d[k] for k in ("idepth_min_stereo", "idepth_max_stereo", "idepth_stereo", "lastTraceUV")]


def test_per_ctx_derived_copies(A, B):
    """sdso_trace_stereo_batch reads plane0, which every ctx builds for itself: first on B's imported pair, then on A's own"""
    pr = synth.stereo_problem(w=W, h=H, npts=400, seed=4031)
    A.upload_pyramid(540, [np.ascontiguousarray(pr["pyr_l"][0])]); A.upload_pyramid(541, [np.ascontiguousarray(pr["pyr_r"][0])])
    hs = [A.export_pyramid(s) for s in (540, 541)]
    for h, s in zip(hs, (49, 50)):
        B.import_pyramid(s, h)
        h.release()
    got = _trace(B, pr, 49, 50)
    want = _trace(A, pr, 540, 541)
    assert (want[2] == 0).sum() > 100
    for g, w in zip(got, want):
        assert np.array_equal(TC.bits(g), TC.bits(w))
    for c, s in ((A, 540), (A, 541), (B, 49), (B, 50)):
        c.check(c.L.sdso_release_pyramid(c.h, s))


def _eval(ctx, prm, lvl, ref, frame, n):
    ev = abi.TrackEval()
    T = (np.eye(3), np.array([0.01, -0.005, 0.008]))
    ctx.L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(abi.SE3.from_Rt(*T)), C.byref(abi.Aff(0.01, 0.5)), 1.0, C.byref(ev))
    Hm, b, res, nw, mask = np.zeros(64), np.zeros(8), np.zeros(6), C.c_int(-1), np.zeros(n, np.uint8)
    ctx.check(ctx.L.sdso_track_calc_res_gs(ctx.h, ref, frame, C.byref(ev), abi.dp(Hm), abi.dp(b), abi.dp(res), C.byref(nw), abi.bp(mask)))
    return Hm.tobytes(), b.tobytes(), res.tobytes(), nw.value, mask.tobytes()


def _track(ctx, prm, ref, frame):
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    ctx.check(ctx.L.sdso_track_newest_coarse(ctx.h, ref, frame, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    R, t = T.Rt()
    return (np.asarray(R).tobytes(), np.asarray(t).tobytes(), aff.a, aff.b, out.good, out.evaluations, list(out.iterations),
            np.array(out.lastResiduals[:]).tobytes(), int(out.point_evals))


def test_template(A, B, windows):
    Wd = windows["nf4"]
    case, up = Wd["case"], Wd["up"]
    L = case["levels"]
    TC.window_route(A, up, REF_A)
    h = A.export_ref(REF_A)
    assert h.info() == (TPL, 0, 2)
    B.import_ref(REF_B, h)
    new_slot = SLOT0["nf4"] + case["nf"] - 2                 # the tracked frame: the keyframe before the newest
    hf = A.export_pyramid(new_slot)
    B.import_pyramid(51, hf)
    hf.release()
    assert same_levels(TC.get_ref(B, REF_B, L), Wd["levels"]) and same_levels(TC.get_ref(A, REF_A, L), Wd["levels"])
    fxs, fys, cxs, cys = synth.level_intrinsics(*Wd["post"]["K32"], L)
    prm = helpers.track_params(dict(levels=L, pyr_ref=case["pyrs"][-1], fx=fxs, fy=fys, cx=cxs, cy=cys))
    for lvl in (0, L - 1):
        n = len(Wd["levels"][lvl]["u"])
        a, b = _eval(A, prm, lvl, REF_A, new_slot, n), _eval(B, prm, lvl, REF_B, 51, n)
        assert a == b and a[3] > 0, lvl
    ra = _track(A, prm, REF_A, new_slot)                     # one ctx after the other, as test_tracking_on_it compares two templates
    rb = _track(B, prm, REF_B, 51)
    assert ra == rb and ra[5] > 0 and ra[8] > 0
    h.release()
    B.check(B.L.sdso_release_pyramid(B.h, 51))


def test_template_frozen(A, B, windows):
    """continues test_template's state where it can, and builds its own where it cannot"""
    W4, W8 = windows["nf4"], windows["nf8"]
    L = W4["case"]["levels"]
    TC.window_route(A, W4["up"], REF_A)
    h = A.export_ref(REF_A)
    B.import_ref(REF_B, h)
    before = A.slot_buffers(TPL, REF_A)[0]
    TC.window_route(A, W8["up"], REF_A)                      # fewer points: the `cap` test alone would keep the buffers
    after, view = A.slot_buffers(TPL, REF_A)
    assert not view and not set(before[:L]) & set(after[:L])
    assert same_levels(TC.get_ref(B, REF_B, L), W4["levels"]) and same_levels(TC.get_ref(A, REF_A, L), W8["levels"])
    h.release()
    # sdso_track_set_ref on one level of an exported template: the other levels stay what they were, on both sides
    h = A.export_ref(REF_A)
    B.import_ref(REF_B + 1, h)
    lv = W4["levels"][1]
    A.check(A.L.sdso_track_set_ref(A.h, REF_A, 1, len(lv["u"]), *[abi.fp(lv[k]) for k in TC.KEYS]))
    assert same_levels(TC.get_ref(B, REF_B + 1, L), W8["levels"]) and same_levels(TC.get_ref(B, REF_B, L), W4["levels"])
    assert same_levels(TC.get_ref(A, REF_A, L), [W8["levels"][0], lv] + W8["levels"][2:])
    # ... and by the importer
    lv0 = W8["levels"][0]
    B.check(B.L.sdso_track_set_ref(B.h, REF_B, 0, len(lv0["u"]), *[abi.fp(lv0[k]) for k in TC.KEYS]))
    assert same_levels(TC.get_ref(B, REF_B, L), [lv0] + W4["levels"][1:])
    assert same_levels(TC.get_ref(B, REF_B + 1, L), W8["levels"])
    h.release()
    for s in (REF_B, REF_B + 1):
        B.check(B.L.sdso_track_release_ref(B.h, s))


def test_counts_in_flight(A, B, windows):
    Wd = windows["nf4"]
    rc, _, _, _ = TC.window_call(A, Wd["up"], REF_A + 3, want=False)   # enqueue-only: the counts are on their way
    A.check(rc)
    h = A.export_ref(REF_A + 3)
    B.import_ref(REF_B + 2, h)
    h.release()
    got = TC.get_ref(B, REF_B + 2, Wd["case"]["levels"])
    assert [len(g["u"]) for g in got] == [len(g["u"]) for g in Wd["levels"]] and same_levels(got, Wd["levels"])
    B.check(B.L.sdso_track_release_ref(B.h, REF_B + 2))
    A.check(A.L.sdso_track_release_ref(A.h, REF_A + 3))


def test_refusals(A, B, windows, images):
    Lb = A.L
    Wd = windows["nf4"]

    def refused(ctx, rc, code=ERR_ARG):
        assert rc == code, rc
        assert Lb.sdso_last_error(ctx.h if ctx else None)

    Cs.make_pyramid(A, 550, images["one"]["img"])
    A.keep_depth_map(True)
    try:
        TC.window_route(A, Wd["up"], REF_A + 4)
    finally:
        A.keep_depth_map(False)
    out = C.c_void_p()
    hp, ht = A.export_pyramid(550), A.export_ref(REF_A + 4)
    # null arguments
    refused(A, Lb.sdso_pyramid_export(A.h, 550, None)); refused(A, Lb.sdso_track_export_ref(A.h, REF_A + 4, None))
    refused(B, Lb.sdso_pyramid_import(B.h, 52, None)); refused(B, Lb.sdso_track_import_ref(B.h, REF_B + 3, None))
    refused(None, Lb.sdso_pyramid_export(None, 550, C.byref(out))); refused(None, Lb.sdso_track_export_ref(None, REF_A + 4, C.byref(out)))
    refused(None, Lb.sdso_pyramid_import(None, 52, hp.h)); refused(None, Lb.sdso_track_import_ref(None, REF_B + 3, ht.h))
    assert Lb.sdso_shared_info(None, None, None, None) == ERR_ARG
    Lb.sdso_shared_release(None)
    # unknown slots
    refused(A, Lb.sdso_pyramid_export(A.h, 559, C.byref(out))); refused(A, Lb.sdso_track_export_ref(A.h, 559, C.byref(out)))
    assert not out.value
    # a handle of the other kind
    refused(B, Lb.sdso_pyramid_import(B.h, 52, ht.h)); refused(B, Lb.sdso_track_import_ref(B.h, REF_B + 3, hp.h))
    assert hp.info() == (PYR, 0, 2) and ht.info() == (TPL, 0, 2)       # nothing was taken
    assert Lb.sdso_download_pyramid_level(B.h, 52, 0, None) == ERR_ARG  # ... and nothing installed
    # another device
    import torch
    if torch.cuda.device_count() > 1:
        D = abi.Context(1)
        try:
            refused(D, Lb.sdso_pyramid_import(D.h, 1, hp.h)); refused(D, Lb.sdso_track_import_ref(D.h, 1, ht.h))
        finally:
            D.close()
    # what does not travel with a template: the kept level-0 map and the STEP1 records
    A.depth_image(REF_A + 4, Wd["up"]["left"], W, H)
    assert len(TC.ref_points(A, REF_A + 4)["point"]) > 100
    B.import_ref(REF_B + 3, ht)
    hl = A.export_pyramid(Wd["up"]["left"])
    B.import_pyramid(52, hl)
    hl.release()
    n = C.c_int(-1)
    refused(B, Lb.sdso_track_depth_image(B.h, REF_B + 3, 52, None, None, None, None, None), ERR_STATE)
    refused(B, Lb.sdso_track_get_ref_points(B.h, REF_B + 3, C.byref(n), None, None, None, None, None, None, None, None), ERR_STATE)
    # ... also where the importing slot had both of its own before
    A.keep_depth_map(True)
    try:
        TC.window_route(A, Wd["up"], REF_A + 5)
    finally:
        A.keep_depth_map(False)
    A.import_ref(REF_A + 5, ht)
    refused(A, Lb.sdso_track_depth_image(A.h, REF_A + 5, Wd["up"]["left"], None, None, None, None, None), ERR_STATE)
    refused(A, Lb.sdso_track_get_ref_points(A.h, REF_A + 5, C.byref(n), None, None, None, None, None, None, None, None), ERR_STATE)
    assert same_levels(TC.get_ref(A, REF_A + 5, Wd["case"]["levels"]), Wd["levels"])
    A.depth_image(REF_A + 4, Wd["up"]["left"], W, H)                   # the builder's own still answer
    assert len(TC.ref_points(A, REF_A + 4)["point"]) > 100
    hp.release(); ht.release()
    for s in (REF_A + 4, REF_A + 5):
        A.check(A.L.sdso_track_release_ref(A.h, s))
    B.check(B.L.sdso_track_release_ref(B.h, REF_B + 3))
    B.check(B.L.sdso_release_pyramid(B.h, 52)); A.check(A.L.sdso_release_pyramid(A.h, 550))


def test_unshared_paths_untouched(A, windows, images):
    """no export anywhere near these slots: a rebuild lands in the same device buffers, as it always did"""
    Cs.make_pyramid(A, 560, images["one"]["img"])
    p0 = A.slot_buffers(PYR, 560)
    Cs.make_pyramid(A, 560, images["two"]["img"])
    A.upload_pyramid(560, [lv[0] for lv in images["one"]["pyr"]])
    assert A.slot_buffers(PYR, 560) == p0 and not p0[1] and all(p0[0][:3]) and not any(p0[0][3:])
    L = windows["nf4"]["case"]["levels"]
    TC.window_route(A, windows["nf4"]["up"], REF_A + 6)
    r0 = A.slot_buffers(TPL, REF_A + 6)
    TC.window_route(A, windows["nf8"]["up"], REF_A + 6)
    TC.window_route(A, windows["nf4"]["up"], REF_A + 6)
    assert A.slot_buffers(TPL, REF_A + 6) == r0 and not r0[1] and all(r0[0][:L])
    # an export taken afterwards views those very buffers
    hp, ht = A.export_pyramid(560), A.export_ref(REF_A + 6)
    assert A.slot_buffers(PYR, 560) == (p0[0], True) and A.slot_buffers(TPL, REF_A + 6) == (r0[0], True)
    assert hp.info() == (PYR, 0, 2) and ht.info() == (TPL, 0, 2)
    hp.release(); ht.release()
    A.check(A.L.sdso_release_pyramid(A.h, 560)); A.check(A.L.sdso_track_release_ref(A.h, REF_A + 6))
