"""The device-resident immature-point set (sdso_imm_*) against its CPU statement (tests/immature_ref.py), bit for bit: every output is a
decision, an integer, or a float produced per point in a fixed operation order, so no tolerance is involved anywhere.

One sequence runs once per module on the device and on the statement (fixture `seq`); the tests assert on what it recorded."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_cases as Cs
import immature_ref as R
import synth

pytestmark = pytest.mark.gpu
SLOT_HOST, SLOT_L, SLOT_R, SLOT_CRAFT, SLOT_SEL = 900, 910, 920, 930, 931   # host k, frame k left / right
ERR_ARG, ERR_STATE = -1, -4


def _geoms(named):
    G = (abi.ImmGeom * max(1, len(named)))()
    for i, (hid, g) in enumerate(named):
        G[i].host_id = hid
        for k in ("KRKi", "Kt", "aff", "KRi", "t"):
            getattr(G[i], k)[:] = [float(x) for x in g[k]]
    return G


def _trace(ctx, case, k, named, nonkey=True, counts=True):
    c = np.full(abi.IMM_NCOUNTS, -1, np.int32)
    rc = ctx.L.sdso_imm_trace(ctx.h, SLOT_L + k, SLOT_R + k if nonkey else -1, len(named), _geoms(named), abi.fp(case["K4"]), abi.fp(case["Ki"]),
                              case["baseline"], abi.ip(c) if counts else None)
    return rc, c


def _old_entry_points(ctx, case):
    """one sdso_trace_on_batch and one sdso_stereo_match_batch call on arrays of their own"""
    rs = np.random.RandomState(3)
    n = 500
    u = rs.randint(20, Cs.W - 20, n).astype(np.float32); v = rs.randint(20, Cs.H - 20, n).astype(np.float32)
    col, wgt, gH, eth = [np.zeros(s, np.float32) for s in ((n, 8), (n, 8), (n, 4), (n,))]
    ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, SLOT_HOST, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
    P, d = abi.make_trace_points(n, u, v, col, wgt, gH, eth)
    g = case["frames"][0]["geom"][0]
    G = abi.TraceGeom(); G.KRKi[:] = [float(x) for x in g["KRKi"]]; G.Kt[:] = [float(x) for x in g["Kt"]]; G.aff[:] = [float(x) for x in g["aff"]]
    st = np.zeros(n, np.uint8)
    ctx.check(ctx.L.sdso_trace_on_batch(ctx.h, SLOT_L, 1, C.byref(G), abi.ip(np.zeros(n, np.int32)), C.byref(P), abi.bp(st)))
    M = abi.StereoMatch()
    out = dict(status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), idepth_stereo=np.zeros(n, np.float32), idepth_min_out=np.zeros(n, np.float32),
               idepth_max_out=np.zeros(n, np.float32), fwd_uv=np.zeros((n, 2), np.float32), back_uv=np.zeros((n, 2), np.float32))
    M.n = n; M.u = abi.fp(u); M.v = abi.fp(v)
    abi.bind(M, out)
    ctx.check(ctx.L.sdso_stereo_match_batch(ctx.h, SLOT_L, SLOT_R, abi.fp(case["K4"]), case["baseline"], 1, C.byref(M)))
    good = out["status_fwd"] == 0
    for k in ("idepth_stereo", "idepth_min_out", "idepth_max_out"):     # defined where the forward trace is GOOD
        out[k] = out[k][good]
    out["back_uv"] = out["back_uv"][out["status_back"] != 255]
    return dict(trace_on=dict(d, status=st), match=out)


@pytest.fixture(scope="module")
def seq(gpu_ctx, oracle):
    ctx, L = gpu_ctx, gpu_ctx.L
    case = Cs.window_case()
    craft = Cs.crafted_map_case()
    rec = dict(case=case)
    hosts, frames = case["hosts"], case["frames"]
    ids = (10, 11, 12, 13)
    try:
        for k, h_ in enumerate(hosts[:3]):
            ctx.upload_pyramid(SLOT_HOST + k, [h_["img"]])
        for k, F in enumerate(frames):
            ctx.upload_pyramid(SLOT_L + k, [F["left"]]); ctx.upload_pyramid(SLOT_R + k, [F["right"]])
        rec["old_before"] = _old_entry_points(ctx, case)

        # ---- 1. add_frame: crafted host map; the NULL-map route after sdso_pixel_select
        ctx.upload_pyramid(SLOT_CRAFT, [craft["img"]])
        n = C.c_int(-1)
        ctx.check(L.sdso_imm_add_frame(ctx.h, 50, SLOT_CRAFT, abi.fp(craft["map"]), C.byref(n)))
        rec["craft"] = (n.value, ctx.imm_get(50), R.add_frame(oracle, craft["img"], craft["map"]), int((craft["map"][3:Cs.H - 4, 3:Cs.W - 4] != 0).sum()))
        rec["null_without_select"] = L.sdso_imm_add_frame(ctx.h, 53, SLOT_CRAFT, None, None)
        pyr = synth.make_pyramid(np.ascontiguousarray(hosts[1]["img"][..., 0]))
        ctx.upload_pyramid(SLOT_SEL, pyr)
        pot = C.c_int(3); num = C.c_int(0)
        sel_map = np.zeros((Cs.H, Cs.W), np.float32)
        ctx.check(L.sdso_pixel_select(ctx.h, SLOT_SEL, 600.0, 1, 1.0, C.byref(pot), abi.fp(sel_map), C.byref(num)))
        rec["null_other_slot"] = L.sdso_imm_add_frame(ctx.h, 53, SLOT_CRAFT, None, None)
        ctx.check(L.sdso_imm_add_frame(ctx.h, 51, SLOT_SEL, None, None))          # enqueue only
        ctx.check(L.sdso_imm_add_frame(ctx.h, 52, SLOT_SEL, abi.fp(sel_map), None))
        rec["select"] = (num.value, sel_map, ctx.imm_get(51), ctx.imm_get(52), R.add_frame(oracle, pyr[0], sel_map))
        ctx.upload_pyramid(SLOT_SEL, pyr)                                          # the slot takes an image anew: the kept map is no longer its map
        rec["null_after_upload"] = L.sdso_imm_add_frame(ctx.h, 53, SLOT_SEL, None, None)
        for hid in (50, 51, 52):
            ctx.check(L.sdso_imm_release_host(ctx.h, hid))

        # ---- 2. the window: four hosts, frames non-key, non-key (g2o refinement, host 11 not named), key
        ref = []
        rec["added"] = []
        for k, h_ in enumerate(hosts):
            n = C.c_int(-1)
            ctx.check(L.sdso_imm_add_frame(ctx.h, ids[k], SLOT_HOST + (k if k < 3 else 0), abi.fp(h_["map"]), C.byref(n) if k != 1 else None))
            ref.append(R.add_frame(oracle, h_["img"], h_["map"]))
            rec["added"].append(n.value)
        get_all = lambda: [ctx.imm_get(i) for i in ids]
        snap = lambda: [{k: v.copy() for k, v in S.items()} for S in ref]
        rec["after_add"] = (get_all(), snap())
        rec["frames"] = []
        plan = ((0, (0, 1, 2, 3), True, 0), (1, (0, 2, 3), True, 1), (2, (3, 2, 1, 0), False, 0))
        for k, who, nonkey, gn in plan:
            if k == 1:
                rec["old_between"] = _old_entry_points(ctx, case)
            ctx.check(L.sdso_trace_set_gn_mode(ctx.h, gn))
            rc, c = _trace(ctx, case, k, [(ids[j], frames[k]["geom"][j]) for j in who], nonkey)
            ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 0))
            ctx.check(rc)
            cr, _, _ = R.trace(oracle, [(ref[j], frames[k]["geom"][j]) for j in who], frames[k]["left"], frames[k]["right"] if nonkey else None, case["K4"],
                               case["Ki"], case["baseline"], gn)
            rec["frames"].append((c, cr, get_all(), snap()))

        # ---- 4. refusals leave the set as it was
        before = get_all()
        g0 = frames[3]["geom"]
        rec["refusals"] = dict(
            unknown=_trace(ctx, case, 3, [(ids[0], g0[0]), (99, g0[1])])[0],
            twice=_trace(ctx, case, 3, [(ids[0], g0[0]), (ids[1], g0[1]), (ids[0], g0[0])])[0],
            wrong_n=L.sdso_imm_remove(ctx.h, ids[0], len(ref[0]["u"]) - 1, abi.bp(np.zeros(len(ref[0]["u"]), np.uint8))),
            occupied=L.sdso_imm_add_frame(ctx.h, ids[1], SLOT_HOST, abi.fp(hosts[0]["map"]), None),
            get_unknown=L.sdso_imm_get(ctx.h, 99, C.byref(abi.TracePoints()), None))
        rec["refusals_state"] = (before, get_all())

        # ---- 3. removal (the last entry, a run at the back, some in between), one more non-key frame, release of a host
        n0 = len(ref[0]["u"])
        flags = np.zeros(n0, np.uint8)
        flags[-1] = 1; flags[-12:-3] = 1; flags[5::37] = 1
        ctx.check(L.sdso_imm_remove(ctx.h, ids[0], n0, abi.bp(flags)))
        R.remove(ref[0], flags)
        ctx.check(L.sdso_imm_remove(ctx.h, ids[2], 1, abi.bp(np.zeros(1, np.uint8))))      # nothing flagged
        rec["removed"] = (int(flags.sum()), get_all(), snap())
        rc, _ = _trace(ctx, case, 3, [(ids[j], g0[j]) for j in range(4)], True, counts=False)
        ctx.check(rc)
        R.trace(oracle, [(ref[j], g0[j]) for j in range(4)], frames[3]["left"], frames[3]["right"], case["K4"], case["Ki"], case["baseline"])
        rec["frame4"] = (get_all(), snap())
        ctx.check(L.sdso_imm_release_host(ctx.h, ids[1]))
        n = C.c_int(-1)
        ctx.check(L.sdso_imm_count(ctx.h, ids[1], C.byref(n)))
        rec["released"] = (n.value, [ctx.imm_get(i) for i in (ids[0], ids[2], ids[3])], [snap()[j] for j in (0, 2, 3)])
        ctx.check(L.sdso_imm_remove(ctx.h, ids[2], 1, abi.bp(np.ones(1, np.uint8))))       # the host's only point
        rec["emptied"] = ctx.imm_get(ids[2])
    finally:
        L.sdso_trace_set_gn_mode(ctx.h, 0)
        for hid in (50, 51, 52, 53) + ids:
            L.sdso_imm_release_host(ctx.h, hid)
        for s in [SLOT_HOST + k for k in range(3)] + [SLOT_L + k for k in range(4)] + [SLOT_R + k for k in range(4)] + [SLOT_CRAFT, SLOT_SEL]:
            L.sdso_release_pyramid(ctx.h, s)
    return rec


def _assert_same(got, want):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        assert R.same(a, b) is None, "host %d: %s differs" % (j, R.same(a, b))


def test_add_frame_from_a_crafted_map(seq):
    n, got, want, ncand = seq["craft"]
    assert n == len(want["u"]) and 0 < ncand - n                   # at least one point dropped for energyTH
    assert R.same(got, want) is None, R.same(got, want)


def test_add_frame_from_the_selector_map(seq):
    num, sel_map, from_null, from_host, want = seq["select"]
    assert num == int((sel_map != 0).sum()) and len(want["u"]) > 300
    assert R.same(from_null, want) is None and R.same(from_host, want) is None
    assert seq["null_without_select"] == ERR_STATE and seq["null_other_slot"] == ERR_STATE and seq["null_after_upload"] == ERR_STATE


def test_window_hosts_hold_their_points(seq):
    assert seq["added"] == [Cs.HOST_POINTS[0], -1, Cs.HOST_POINTS[2], 0]       # host 11 was added without reading the count
    got, want = seq["after_add"]
    assert [len(S["u"]) for S in got] == list(Cs.HOST_POINTS) + [0]
    _assert_same(got, want)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_three_frames_on_the_resident_set(seq, k):
    c, cr, got, want = seq["frames"][k]
    print("frame", k + 1, "counts", c, "statement", cr)
    assert np.array_equal(c, cr)
    _assert_same(got, want)
    if k == 1:      # host 11 was not named: what frame 1 left
        assert R.same(got[1], seq["frames"][0][2][1]) is None
    if k == 2:      # the key form runs no stereo step
        assert (c[6:] == 0).all() and c[:6].sum() == sum(Cs.HOST_POINTS)
    else:
        assert c[R.C_UPDATED] > 0 and c[R.C_FWD_GOOD] >= c[R.C_UPDATED] + c[R.C_STEREO_OUTLIER]


def test_remove_then_trace_then_release(seq):
    nflag, got, want = seq["removed"]
    assert len(got[0]["u"]) == Cs.HOST_POINTS[0] - nflag
    _assert_same(got, want)
    _assert_same(*seq["frame4"])
    n, got, want = seq["released"]
    assert n == 0
    _assert_same(got, want)
    assert len(seq["emptied"]["u"]) == 0


def test_refusals_leave_the_set_alone(seq):
    r = seq["refusals"]
    assert r == dict(unknown=ERR_ARG, twice=ERR_ARG, wrong_n=ERR_ARG, occupied=ERR_ARG, get_unknown=ERR_ARG), r
    _assert_same(*seq["refusals_state"])


def test_old_entry_points_are_undisturbed(seq):
    a, b = seq["old_before"], seq["old_between"]
    for part in ("trace_on", "match"):
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k], equal_nan=a[part][k].dtype != np.uint8), (part, k)
    assert (a["trace_on"]["status"] == 0).sum() > 50 and (a["match"]["status_fwd"] == 0).sum() > 50
