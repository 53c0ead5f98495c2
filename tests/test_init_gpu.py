"""The stereo initialiser on the device (sdso_init_*) against its CPU statement (tests/init_ref.py): Pnts, counts, PointHessian records and
their order.  Every float is compared as bits (NaN equals NaN): no tolerance is involved anywhere.

One sequence runs once per module on the device (fixture `seq`) and the statement once on the CPU oracle (fixture `ref`); the tests assert
on what they recorded.  The conditions these cases rely on are asserted on the CPU in tests/test_init_ref.py."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_ref as R
import init_cases as IC
import init_ref as IR

pytestmark = pytest.mark.gpu
f32 = np.float32
SLOT_L6, SLOT_R6, SLOT_L3, SLOT_R3, SLOT_CRAFT, SLOT_TINY_L, SLOT_TINY_R = 960, 961, 962, 963, 964, 965, 966
HOST_BEFORE = 75                               # a group of the resident immature set, made before anything else
ERR_ARG, ERR_STATE = -1, -4
BIG, SMALL = IC.SIZES


@pytest.fixture(scope="module")
def ref(oracle):
    """the CPU statement of every case, computed once"""
    out = {}
    for size in IC.SIZES:
        P = IC.stereo_pair(*size)
        made, m = IR.select(oracle, P["pyr_left"], IC.density(*size))
        out[size] = dict(made=made, map=m, state=IR.set_first_with(m, IR.trace_first(oracle, P["pyr_left"][0], P["right"], P["K4"], P["baseline"])))
    P = IC.stereo_pair(*SMALL)
    out["gn1"] = IR.set_first_with(out[SMALL]["map"], IR.trace_first(oracle, P["pyr_left"][0], P["right"], P["K4"], P["baseline"], gn_mode=1))
    c = IC.crafted_case()
    trace = IR.trace_first(oracle, c["left"], c["right"], c["K4"], c["baseline"])
    out["craft"] = IR.set_first_with(c["map"], trace)
    out["single"] = IR.set_first_with(IC.single_entry_map(*BIG), trace)
    n = out[BIG]["state"]["n"]
    out["keep"] = IC.keep_flags(n, 5, IC.DESIRED_POINT_DENSITY / n)       # keepPercentage of FullSystem.cpp:1525
    out["keep2"] = IC.keep_flags(n, 6, 0.5)
    return out


def _older_entry_points(ctx, P, slot_l, slot_r):
    """setFirstStereo's loop composed from sdso_pixel_select (with the map download), sdso_immature_init_batch and sdso_trace_stereo_batch,
    the rules in NumPy -> the state of init_ref.set_first_with"""
    w, h = P["w"], P["h"]
    m = np.zeros((h, w), f32)
    pot, num = C.c_int(3), C.c_int(0)
    ctx.check(ctx.L.sdso_pixel_select(ctx.h, slot_l, IC.density(w, h), 1, 2.0, C.byref(pot), abi.fp(m), C.byref(num)))

    def trace(u, v):
        n = len(u)
        col, wgt, gH, eth = [np.zeros(s, f32) for s in ((n, 8), (n, 8), (n, 4), (n,))]
        ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, slot_l, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
        T, d = abi.make_trace_points(n, u, v, col, wgt, gH, eth)
        st = np.zeros(n, np.uint8)
        ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, slot_r, abi.fp(P["K4"]), P["baseline"], 1, C.byref(T), abi.bp(st)))
        return dict(status=st, energyTH=eth, idepth_min=d["idepth_min_stereo"], idepth_max=d["idepth_max_stereo"], idepth_stereo=d["idepth_stereo"], color=col,
                    weights=wgt)
    return num.value, IR.set_first_with(m, trace)


def _run(ctx, slot_l, slot_r, P, selection_map, keep, cap, read=True):
    """set_first_stereo, get_pnts, from_initializer, get_points -> what they returned; cap sizes the caller's arrays where nothing is read"""
    n, counts = ctx.init_set_first_stereo(slot_l, slot_r, P["K4"], P["baseline"], selection_map, read=read)
    pnts = ctx.init_get_pnts(cap if n is None else n)
    npts, c4 = ctx.init_from_initializer(keep, read=read)
    points = ctx.init_get_points(len(pnts["u"]) if npts is None else npts)
    return dict(n=n, counts=counts, pnts=pnts, npts=npts, c4=c4, points=points)


def _raw_codes(ctx):
    L = ctx.L
    return dict(from_initializer=L.sdso_init_from_initializer(ctx.h, None, None, None), get_pnts=L.sdso_init_get_pnts(ctx.h, C.byref(abi.InitPnts())),
                get_points=L.sdso_init_get_points(ctx.h, C.byref(abi.InitPoints())))


@pytest.fixture(scope="module")
def seq(gpu_ctx, ref):
    ctx, L = gpu_ctx, gpu_ctx.L
    P6, P3, craft = IC.stereo_pair(*BIG), IC.stereo_pair(*SMALL), IC.crafted_case()
    n6 = ref[BIG]["state"]["n"]
    rec = {}
    try:
        ctx.check(L.sdso_init_release(ctx.h))
        ctx.upload_pyramid(SLOT_L6, P6["pyr_left"]); ctx.upload_pyramid(SLOT_R6, [P6["right"]])
        ctx.upload_pyramid(SLOT_L3, P3["pyr_left"]); ctx.upload_pyramid(SLOT_R3, [P3["right"]])
        ctx.upload_pyramid(SLOT_CRAFT, [craft["left"]])
        tiny = [np.zeros((s, s, 3), f32) for s in (24, 12, 8)]      # three levels (none under 8 x 8), yet smaller than one 32 x 32 cell
        ctx.upload_pyramid(SLOT_TINY_L, tiny); ctx.upload_pyramid(SLOT_TINY_R, tiny[:1])
        ctx.check(L.sdso_imm_add_frame(ctx.h, HOST_BEFORE, SLOT_CRAFT, abi.fp(craft["map"]), None))
        rec["imm_before"] = ctx.imm_get(HOST_BEFORE)
        rec["before_any"] = _raw_codes(ctx)

        # ---- 640 x 480: the library's own selection; STEP 3 twice with different flags, the Pnts read in between
        n, counts = ctx.init_set_first_stereo(SLOT_L6, SLOT_R6, P6["K4"], P6["baseline"])
        rec["points_before_step3"] = L.sdso_init_get_points(ctx.h, C.byref(abi.InitPoints()))
        A = dict(n=n, counts=counts, pnts=ctx.init_get_pnts(n))
        A["npts"], A["c4"] = ctx.init_from_initializer(ref["keep"])
        A["points"] = ctx.init_get_points(A["npts"])
        A["pnts_between"] = ctx.init_get_pnts(n)
        A["npts2"], A["c4_2"] = ctx.init_from_initializer(ref["keep2"])
        A["points2"] = ctx.init_get_points(A["npts2"])
        A["pnts_after"] = ctx.init_get_pnts(n)
        rec["own_map"] = A
        # ---- again with the oracle's map passed in; then the enqueue-only forms followed by the get calls
        rec["host_map"] = _run(ctx, SLOT_L6, SLOT_R6, P6, ref[BIG]["map"], ref["keep"], n6)
        rec["enqueue_only"] = _run(ctx, SLOT_L6, SLOT_R6, P6, ref[BIG]["map"], ref["keep"], n6 + 9, read=False)
        rec["older"] = _older_entry_points(ctx, P6, SLOT_L6, SLOT_R6)
        # ---- a crafted map, one entry, no entry in the walked area
        rec["craft"] = _run(ctx, SLOT_CRAFT, SLOT_R6, P6, craft["map"], None, 0)
        rec["single"] = _run(ctx, SLOT_CRAFT, SLOT_R6, P6, IC.single_entry_map(*BIG), None, 0)
        rec["none"] = _run(ctx, SLOT_CRAFT, SLOT_R6, P6, IC.border_only_map(*BIG), None, 0)
        rec["none_enqueued"] = _run(ctx, SLOT_CRAFT, SLOT_R6, P6, IC.border_only_map(*BIG), None, 5, read=False)
        # ---- 320 x 240, keep = NULL: a second set_first_stereo replaces the state; then refinement mode 1
        ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 1))
        rec["gn1"] = _run(ctx, SLOT_L3, SLOT_R3, P3, None, None, 0)
        ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 0))
        rec["small"] = _run(ctx, SLOT_L3, SLOT_R3, P3, None, None, 0)

        # ---- every refusal leaves the state readable and unchanged
        K6, K3 = abi.fp(P6["K4"]), abi.fp(P3["K4"])
        first = lambda l, r, K, m=None: L.sdso_init_set_first_stereo(ctx.h, l, r, K, P6["baseline"], m, None, None)
        rec["refusals"] = dict(unknown_frame=first(9999, SLOT_R6, K6), unknown_right=first(SLOT_L6, 9999, K6), other_size=first(SLOT_L3, SLOT_R6, K3),
                               null_K=first(SLOT_L6, SLOT_R6, None), levels=first(SLOT_CRAFT, SLOT_R6, K6),
                               no_selector_state=first(SLOT_TINY_L, SLOT_TINY_R, K3))
        n3 = rec["small"]["n"]
        rec["after_refusals"] = dict(pnts=ctx.init_get_pnts(n3), points=ctx.init_get_points(rec["small"]["npts"]))
        rec["imm_after"] = ctx.imm_get(HOST_BEFORE)
        ctx.check(L.sdso_init_release(ctx.h))
        rec["after_release"] = _raw_codes(ctx)
    finally:
        L.sdso_trace_set_gn_mode(ctx.h, 0)
        L.sdso_init_release(ctx.h)
        L.sdso_imm_release_host(ctx.h, HOST_BEFORE)
        for s in (SLOT_L6, SLOT_R6, SLOT_L3, SLOT_R3, SLOT_CRAFT, SLOT_TINY_L, SLOT_TINY_R):
            L.sdso_release_pyramid(ctx.h, s)
    return rec


def _assert_run(got, state, keep=None, read=True):
    """one set_first_stereo + from_initializer run against the statement"""
    want = IR.from_initializer(state, keep)
    if read:
        print("counts", got["counts"], got["c4"], "statement", state["counts"], want["counts"])
        assert got["n"] == state["n"] and np.array_equal(got["counts"], state["counts"])
        assert got["npts"] == want["n"] and np.array_equal(got["c4"], want["counts"])
    assert IR.same(got["pnts"], state["pnts"], IR.PNT) is None, IR.same(got["pnts"], state["pnts"], IR.PNT)
    assert IR.same(got["points"], want["points"], IR.POINT) is None, IR.same(got["points"], want["points"], IR.POINT)


def test_own_selection_at_640x480(seq, ref):
    A, S = seq["own_map"], ref[BIG]["state"]
    assert A["counts"][0] == ref[BIG]["made"] == 9205 and A["n"] == 9205 and A["n"] % 64 and A["n"] % 256
    _assert_run(A, S, ref["keep"])
    assert 0 < A["c4"][1] and 0 < A["c4"][2] and 0 < A["npts"] < 0.3 * A["n"]


def test_step_3_twice_with_other_flags_leaves_the_pnts(seq, ref):
    A, S = seq["own_map"], ref[BIG]["state"]
    want2 = IR.from_initializer(S, ref["keep2"])
    assert A["npts2"] == want2["n"] != A["npts"] and np.array_equal(A["c4_2"], want2["counts"])
    assert IR.same(A["points2"], want2["points"], IR.POINT) is None
    for k in ("pnts_between", "pnts_after"):
        assert IR.same(A[k], S["pnts"], IR.PNT) is None
    assert seq["points_before_step3"] == ERR_STATE


def test_the_oracles_map_passed_in(seq, ref):
    _assert_run(seq["host_map"], ref[BIG]["state"], ref["keep"])


def test_enqueue_only_forms_then_the_get_calls(seq, ref):
    got = seq["enqueue_only"]
    assert got["n"] is None and len(got["pnts"]["u"]) == ref[BIG]["state"]["n"]          # out->n is the library's, not the caller's capacity
    _assert_run(got, ref[BIG]["state"], ref["keep"], read=False)
    got = seq["none_enqueued"]
    assert len(got["pnts"]["u"]) == 0 and len(got["points"]["u"]) == 0


def test_320x240_with_every_pnt_kept(seq, ref):
    S = ref[SMALL]["state"]
    got = seq["small"]
    assert got["counts"][0] == ref[SMALL]["made"] == 1946 and got["n"] == 1900 < got["counts"][0]   # selected pixels in the excluded border are skipped
    _assert_run(got, S)                                                                            # it replaced the 640 x 480 state
    assert got["c4"][1] == 0 and got["npts"] == 1617 and (got["pnts"]["status"][got["points"]["pnt"]] == R.GOOD).all()


def test_refinement_mode_1(seq, ref):
    _assert_run(seq["gn1"], ref["gn1"])
    assert IR.same(seq["gn1"]["pnts"], seq["small"]["pnts"], IR.PNT) is not None       # the mode is the ctx's, and it matters


def test_crafted_map(seq, ref):
    c, S, got = IC.crafted_case(), ref["craft"], seq["craft"]
    _assert_run(got, S)
    assert got["counts"][0] - got["n"] == len(IC.BORDER(*BIG))
    bad = list(c["bad"])
    assert (got["pnts"]["idepth"][bad] == f32(0.01)).all() and not set(bad) & set(got["points"]["pnt"])   # Pnts all the same, dropped in STEP 3
    assert set(np.unique(got["pnts"]["my_type"])) == {1.0, 2.0, 4.0}


def test_maps_with_one_entry_and_with_none(seq, ref):
    _assert_run(seq["single"], ref["single"])
    assert seq["single"]["n"] == 1 and list(seq["single"]["counts"][:2]) == [1, 1]
    got = seq["none"]
    assert got["n"] == 0 and list(got["counts"]) == [len(IC.BORDER(*BIG)), 0, 0, 0, 0, 0, 0, 0]
    assert got["npts"] == 0 and list(got["c4"]) == [0, 0, 0, 0] and len(got["pnts"]["u"]) == 0 and len(got["points"]["pnt"]) == 0


def test_composition_of_the_older_entry_points_gives_the_same_pnts(seq, ref):
    num, S = seq["older"]
    assert num == ref[BIG]["made"]
    assert IR.same(S["pnts"], seq["own_map"]["pnts"], IR.PNT) is None and np.array_equal(S["counts"], seq["own_map"]["counts"])
    assert IR.same(IR.from_initializer(S, ref["keep"])["points"], seq["own_map"]["points"], IR.POINT) is None


def test_refusals_leave_the_state_readable_and_unchanged(seq):
    r = seq["refusals"]
    assert r == dict(unknown_frame=ERR_ARG, unknown_right=ERR_ARG, other_size=ERR_ARG, null_K=ERR_ARG, levels=ERR_ARG, no_selector_state=ERR_STATE), r
    assert IR.same(seq["after_refusals"]["pnts"], seq["small"]["pnts"], IR.PNT) is None
    assert IR.same(seq["after_refusals"]["points"], seq["small"]["points"], IR.POINT) is None
    want = dict(from_initializer=ERR_STATE, get_pnts=ERR_STATE, get_points=ERR_STATE)
    assert seq["before_any"] == want and seq["after_release"] == want


def test_the_resident_immature_set_is_untouched(seq):
    a, b = seq["imm_before"], seq["imm_after"]
    assert len(a["u"]) > 250 and R.same(a, b) is None, R.same(a, b)
