"""sdso_imm_stereo_match (FullSystem::stereoMatch's loop on a resident group) against its CPU statement (tests/stereo_match_ref.py), bit
for bit: every output is a decision, a count, or a float the trace kernels produce per point in a fixed operation order, and the same
kernels are already held to the same oracle exactly in tests/test_immature_gpu.py.  No tolerance is involved anywhere.

One sequence runs once per module on the device (fixture `seq`); the tests assert on what it recorded."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_cases as Cs
import immature_ref as R
import stereo_match_cases as Ms
import stereo_match_ref as M
import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
SLOT_L, SLOT_R, SLOT_SEL, SLOT_SMALL, SLOT_HOST = 960, 961, 962, 963, 964
IDS = {1037: 70, 259: 71, 1: 72, 0: 73}
ID_SEL, ID_DOC, ID_OTHER = 74, 75, 76
ERR_ARG, ERR_STATE = -1, -4
W, H = Cs.W, Cs.H


def _map_from_device(ctx):
    """the kept map, copied from the pointer sdso_imm_stereo_map_dev returns"""
    ptr, w, h = ctx.imm_stereo_map_dev()
    m = np.full((h, w, 3), -1, f32)
    ctx.sync()
    assert ctx.L.hipMemcpy(C.c_void_p(m.ctypes.data), C.c_void_p(ptr), C.c_size_t(m.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return m


def _match(ctx, c, hid, frame_slot=SLOT_L, **kw):
    return ctx.imm_stereo_match(hid, frame_slot, SLOT_R, c["K4"], c["baseline"], map_wh=(W, H), **kw)


def _raw(ctx, c, hid=IDS[259], frame=SLOT_L, right=SLOT_R, K=True, max_depth=70.0, build_map=1, with_map=False):
    """the bare call, for the refusals -> return code"""
    O, d, counts = ctx.imm_match_arrays(259, W if with_map else 0, H if with_map else 0)
    return ctx.L.sdso_imm_stereo_match(ctx.h, hid, frame, right, abi.fp(c["K4"]) if K else None, c["baseline"], max_depth, build_map, C.byref(O), abi.ip(counts))


def _trace_other(ctx, c, other, snapshot):
    """sdso_imm_trace (non-key) on a group of its own, installed anew from `snapshot` -> (counts, the group afterwards)"""
    ctx.imm_put(ID_OTHER, snapshot, W, H)
    G = (abi.ImmGeom * 1)()
    G[0].host_id = ID_OTHER
    for k in ("KRKi", "Kt", "aff", "KRi", "t"):
        getattr(G[0], k)[:] = [float(x) for x in other["geom"][k]]
    cn = np.full(abi.IMM_NCOUNTS, -1, np.int32)
    ctx.check(ctx.L.sdso_imm_trace(ctx.h, SLOT_L, SLOT_R, 1, G, abi.fp(c["K4"]), abi.fp(other["Ki"]), c["baseline"], abi.ip(cn)))
    got = ctx.imm_get(ID_OTHER)
    ctx.check(ctx.L.sdso_imm_release_host(ctx.h, ID_OTHER))
    return cn, got


def _match_batch(ctx, c):
    """one sdso_stereo_match_batch call on arrays of its own"""
    rs = np.random.RandomState(3)
    n = 500
    u = rs.randint(20, W - 20, n).astype(f32); v = rs.randint(20, H - 20, n).astype(f32)
    out = dict(status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), idepth_stereo=np.zeros(n, f32), idepth_min_out=np.zeros(n, f32),
               idepth_max_out=np.zeros(n, f32), fwd_uv=np.zeros((n, 2), f32), back_uv=np.zeros((n, 2), f32))
    Mb = abi.StereoMatch()
    Mb.n = n; Mb.u = abi.fp(u); Mb.v = abi.fp(v)
    abi.bind(Mb, out)
    ctx.check(ctx.L.sdso_stereo_match_batch(ctx.h, SLOT_L, SLOT_R, abi.fp(c["K4"]), c["baseline"], 1, C.byref(Mb)))
    good = out["status_fwd"] == 0
    for k in ("idepth_stereo", "idepth_min_out", "idepth_max_out"):     # defined where the forward trace is GOOD
        out[k] = out[k][good]
    out["back_uv"] = out["back_uv"][out["status_back"] != 255]
    return out


def _composition(ctx, c, S):
    """the loop through the older device entry points, which run the same kernels: sdso_trace_stereo_batch, sdso_immature_init_batch"""
    def init_right(u, v):
        n = len(u)
        col, wgt, gH, eth = np.zeros((n, 8), f32), np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros(n, f32)
        if n:
            ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, SLOT_R, n, abi.fp(u), abi.fp(v), abi.fp(col), abi.fp(wgt), abi.fp(gH), abi.fp(eth)))
        return col, wgt, gH, eth

    def trace(P, in_right):
        st = np.zeros(P.n, np.uint8)
        if P.n:
            ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, SLOT_R if in_right else SLOT_L, abi.fp(c["K4"]), c["baseline"], 1 if in_right else 0, C.byref(P), abi.bp(st)))
        return st
    return M.match_with(S, W, H, init_right, trace)


def _doctor(S):
    """what a group of sdso_imm_put_host may carry and makeNewTraces never leaves: colours the pyramid would not give, a stored interval,
    a last trace"""
    D = {k: np.array(v, copy=True) for k, v in S.items()}
    ten = np.arange(20, 120, 10)
    D["color"][ten[:5]] += f32(60)                                  # no match in the right image any more
    D["color"][ten[5:]] = D["color"][ten[5:] + 1]                    # a neighbour's patch
    D["idepth_min"][:40] = f32(0.05); D["idepth_max"][:40] = f32(0.2)
    D["lastTraceStatus"][::3] = R.OUTLIER; D["lastTraceStatus"][1::3] = R.GOOD
    D["quality"][::2] = f32(1.5)
    D["lastTraceUV"][:, 0] = D["u"] - f32(7.25); D["lastTraceUV"][:, 1] = D["v"]
    D["lastTracePixelInterval"][:] = f32(2.4)
    return D, ten


@pytest.fixture(scope="module")
def seq(gpu_ctx, oracle):
    ctx, L = gpu_ctx, gpu_ctx.L
    c, other = Ms.pair(), Ms.other_host()
    rec = dict(case=c)
    try:
        fresh = abi.Context(0)
        try:
            O, _, cn = fresh.imm_match_arrays(0)
            p, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
            rec["fresh"] = (L.sdso_imm_stereo_match_fetch(fresh.h, C.byref(O), abi.ip(cn)), L.sdso_imm_stereo_map_dev(fresh.h, C.byref(p), C.byref(w), C.byref(h)))
        finally:
            fresh.close()
        ctx.upload_pyramid(SLOT_L, [c["left"]]); ctx.upload_pyramid(SLOT_R, [c["right"]]); ctx.upload_pyramid(SLOT_HOST, [other["img"]])
        ctx.upload_pyramid(SLOT_SMALL, [np.zeros((H // 2, W // 2, 3), f32)])
        ctx.check(L.sdso_imm_add_frame(ctx.h, ID_OTHER, SLOT_HOST, abi.fp(other["map"]), None))
        other_snapshot = ctx.imm_get(ID_OTHER)
        ctx.check(L.sdso_imm_release_host(ctx.h, ID_OTHER))
        rec["old_before"] = (_match_batch(ctx, c), _trace_other(ctx, c, other, other_snapshot))

        # ---- 1. parity on groups of 1037, 259, 1 and 0 points; the map through out->map and from the device pointer
        ref, want = {}, {}
        rec["parity"] = {}
        for n, hid in IDS.items():
            ctx.check(L.sdso_imm_add_frame(ctx.h, hid, SLOT_L, abi.fp(c["maps"][n]), None))
            ref[n] = R.add_frame(oracle, c["left"], c["maps"][n])
            want[n] = M.stereo_match(oracle, ref[n], c["left"], c["right"], c["K4"], c["baseline"])
            rec["parity"][n] = (_match(ctx, c, hid), _map_from_device(ctx), want[n])

        # ---- 2. the group is untouched; a second call returns the same bytes
        before = ctx.imm_get(IDS[1037])
        first = _match(ctx, c, IDS[1037])
        rec["untouched"] = (before, ctx.imm_get(IDS[1037]), ref[1037], first, _match(ctx, c, IDS[1037]))

        # ---- 3. max_depth
        rec["depth20"] = (_match(ctx, c, IDS[1037], max_depth=20.0), M.stereo_match(oracle, ref[1037], c["left"], c["right"], c["K4"], c["baseline"], max_depth=20.0))

        # ---- 4. enqueue only, another host traced in between, then the fetch
        ctx.check(L.sdso_imm_stereo_match(ctx.h, IDS[1037], SLOT_L, SLOT_R, abi.fp(c["K4"]), c["baseline"], 70.0, 1, None, None))
        between = _trace_other(ctx, c, other, other_snapshot)
        rec["enqueue"] = (ctx.imm_stereo_match_fetch(1037, W, H), between)

        # ---- 5. the selector's own map (sdso_pixel_select + sdso_imm_add_frame(NULL)) against the statement on the oracle's map
        pyr = synth.make_pyramid(np.ascontiguousarray(c["left"][..., 0]))
        ctx.upload_pyramid(SLOT_SEL, pyr)
        pot = C.c_int(3); num = C.c_int(0)
        ctx.check(L.sdso_pixel_select(ctx.h, SLOT_SEL, 600.0, 1, 1.0, C.byref(pot), None, C.byref(num)))
        ctx.check(L.sdso_imm_add_frame(ctx.h, ID_SEL, SLOT_SEL, None, None))
        keep = [np.ascontiguousarray(pyr[l]) for l in range(3)]
        ptrs = (abi.c_float_p * 3)(*[abi.fp(a) for a in keep])
        omap = np.zeros((H, W), f32); opot = C.c_int(3)
        onum = oracle.orc_pixel_select(ptrs, W, H, 600.0, 1, 1.0, C.byref(opot), abi.fp(omap))
        S_sel = R.add_frame(oracle, pyr[0], omap)
        rec["selector"] = (num.value, onum, _match(ctx, c, ID_SEL, frame_slot=SLOT_SEL), M.stereo_match(oracle, S_sel, pyr[0], c["right"], c["K4"], c["baseline"]))

        # ---- 6. a doctored group through sdso_imm_put_host
        D, ten = _doctor(ref[259])
        ctx.imm_put(ID_DOC, D, W, H)
        rec["doctored"] = (_match(ctx, c, ID_DOC), M.stereo_match(oracle, D, c["left"], c["right"], c["K4"], c["baseline"]), ten, ctx.imm_get(ID_DOC), D)

        # ---- 7. the fork's refinement: the composition of the older entry points, which run the same kernels
        ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 1))
        got = _match(ctx, c, IDS[259])
        comp = _composition(ctx, c, ctx.imm_get(IDS[259]))
        ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 0))
        rec["gn1"] = (got, comp)

        # ---- 8. refusals leave the set, the kept results and the kept map alone
        kept = _match(ctx, c, IDS[259])
        state = lambda: (ctx.imm_get(IDS[259]), ctx.imm_stereo_match_fetch(259, W, H), _map_from_device(ctx))
        s0 = state()
        rec["refusals"] = dict(
            host=_raw(ctx, c, hid=999), frame=_raw(ctx, c, frame=998), right=_raw(ctx, c, right=997), frame_size=_raw(ctx, c, frame=SLOT_SMALL),
            right_size=_raw(ctx, c, right=SLOT_SMALL), K=_raw(ctx, c, K=False), depth_zero=_raw(ctx, c, max_depth=0.0), depth_negative=_raw(ctx, c, max_depth=-1.0),
            depth_nan=_raw(ctx, c, max_depth=float("nan")), map_without_build=_raw(ctx, c, build_map=0, with_map=True))
        rec["refusals_state"] = (kept, s0, state())
        # without a map: the per-point results are replaced, the kept map is not
        no_map = ctx.imm_stereo_match(IDS[1], SLOT_L, SLOT_R, c["K4"], c["baseline"])
        O, _, cn = ctx.imm_match_arrays(1, W, H)
        rec["no_map"] = (no_map, L.sdso_imm_stereo_match_fetch(ctx.h, C.byref(O), abi.ip(cn)), _map_from_device(ctx), s0[2])

        rec["old_after"] = (_match_batch(ctx, c), _trace_other(ctx, c, other, other_snapshot))
    finally:
        L.sdso_trace_set_gn_mode(ctx.h, 0)
        for hid in list(IDS.values()) + [ID_SEL, ID_DOC, ID_OTHER]:
            L.sdso_imm_release_host(ctx.h, hid)
        for s in (SLOT_L, SLOT_R, SLOT_SEL, SLOT_SMALL, SLOT_HOST):
            L.sdso_release_pyramid(ctx.h, s)
    return rec


@pytest.mark.parametrize("n", [1037, 259, 1, 0])
def test_parity_with_the_statement(seq, n):
    got, dev_map, want = seq["parity"][n]
    print(n, "counts", got["counts"], "statement", want["counts"])
    assert M.same(got, want) is None, M.same(got, want)
    assert np.array_equal(dev_map, want["map"])
    assert got["counts"][M.C_WALKED] == n and got["counts"][M.C_UNREADABLE] == 0
    if n == 0:
        assert not got["counts"].any() and not got["map"].any() and not dev_map.any()
    if n == 1037:
        assert got["counts"][M.C_ACCEPTED] >= 500 and got["counts"][M.C_FAR] >= 50 and got["counts"][M.C_DEPTH] >= 5


def test_selector_route(seq):
    num, onum, got, want = seq["selector"]
    assert num == onum and want["counts"][M.C_WALKED] > 300 and want["counts"][M.C_ACCEPTED] > 100
    assert M.same(got, want) is None, M.same(got, want)


def test_doctored_group_is_traced_as_it_was_put(seq):
    got, want, ten, stored, D = seq["doctored"]
    assert R.same(stored, D) is None                                # the group holds what was put, before and after the call
    assert M.same(got, want) is None, M.same(got, want)
    plain = seq["parity"][259][0]
    differs = [i for i in ten if any(not np.array_equal(got[k][i], plain[k][i]) for k in M.RESULT)]
    print("doctored points that end differently:", differs)
    assert len(differs) >= 1
    assert (got["status_fwd"] == R.OOB).sum() > (plain["status_fwd"] == R.OOB).sum()      # OUTLIER after OUTLIER is OOB (ImmaturePoint.cpp:417-419)


def test_group_is_untouched_and_the_call_repeatable(seq):
    before, after, ref, first, second = seq["untouched"]
    assert R.same(before, after) is None and R.same(after, ref) is None
    assert M.same(first, second) is None and M.same(first, seq["parity"][1037][2]) is None


def test_max_depth(seq):
    got, want = seq["depth20"]
    base = seq["parity"][1037][0]["counts"]
    assert M.same(got, want) is None, M.same(got, want)
    moved = base[M.C_ACCEPTED] - got["counts"][M.C_ACCEPTED]
    assert moved > 0 and got["counts"][M.C_DEPTH] - base[M.C_DEPTH] == moved


def test_enqueue_only_then_fetch(seq):
    got, (cn, _) = seq["enqueue"]
    assert cn[R.C_FWD_GOOD] > 0 and cn[R.C_UPDATED] > 0            # the trace in between ran the stereo chain on the shared batches
    assert M.same(got, seq["parity"][1037][0]) is None, M.same(got, seq["parity"][1037][0])
    assert seq["fresh"] == (ERR_STATE, ERR_STATE)


def test_refinement_mode_1_is_the_composition_of_the_old_entry_points(seq):
    got, comp = seq["gn1"]
    assert M.same(got, comp) is None, M.same(got, comp)
    assert comp["counts"][M.C_ACCEPTED] > 100
    assert M.same(got, seq["parity"][259][0], M.RESULT) is not None      # the mode is honoured: not the DSO-native result


def test_refusals_leave_everything_alone(seq):
    r = seq["refusals"]
    assert all(v == ERR_ARG for v in r.values()) and len(r) == 10, r
    kept, (g0, f0, m0), (g1, f1, m1) = seq["refusals_state"]
    assert R.same(g0, g1) is None
    assert M.same(f0, kept) is None and M.same(f1, kept) is None
    assert np.array_equal(m0, kept["map"]) and np.array_equal(m1, kept["map"])
    no_map, rc_fetch_map, m2, _ = seq["no_map"]
    assert no_map["counts"][M.C_WALKED] == 1 and rc_fetch_map == ERR_ARG and np.array_equal(m2, m0)


def test_old_entry_points_are_undisturbed(seq):
    (ma, (ca, ga)), (mb, (cb, gb)) = seq["old_before"], seq["old_after"]
    for k in ma:
        assert np.array_equal(ma[k], mb[k], equal_nan=ma[k].dtype != np.uint8), k
    assert np.array_equal(ca, cb) and R.same(ga, gb) is None
    assert (ma["status_fwd"] == 0).sum() > 50 and ca[R.C_UPDATED] > 0
