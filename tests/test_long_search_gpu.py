"""traceStereo / traceOn with searches of more than 64 steps, on the device against the oracle, bit for bit.

Both kernels put one search step on each lane of a wave and take a second pass for steps 64 ... 98; at the image sizes of the other
tests (at most 45 steps) that pass, the merge of a lane's two candidates, the index tie rule across the passes, the second-best scan
over s >= 64 and the 99-step cap never run.  tests/long_search_cases.py has the inputs, test_long_search_ref.py shows on the oracle
alone that they reach that code.  Every output is a decision or a float produced per point in a fixed operation order: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import immature_ref as R
import long_search_cases as Ls

pytestmark = pytest.mark.gpu
SHAPES = {"S1": Ls.S1, "S2": Ls.S2}
SLOT_L, SLOT_R, SLOT_NEW, SLOT_HOST, SLOT_FL, SLOT_FR = 940, 941, 942, 943, 944, 945
HOST_IDS = (60, 61, 62)
PERIODIC_HOST_ID = 63


def _release(ctx, *slots):
    for s in slots:
        ctx.L.sdso_release_pyramid(ctx.h, s)


def _same(got, want, fields=Ls.FIELDS):
    (sg, dg), (so, do) = got, want
    assert np.array_equal(sg, so)
    for k in fields:
        assert np.array_equal(dg[k], do[k], equal_nan=True), k


def _rows(res, rows):
    st, d = res
    return st[rows], {k: d[k][rows] for k in Ls.FIELDS}


def _points(case, init, imin=None, imax=None, rows=slice(None)):
    sl = lambda a: None if a is None else a[rows]
    u = case["u"][rows]
    return abi.make_trace_points(len(u), u, case["v"][rows], *[a[rows] for a in init], sl(imin), sl(imax))


def _gpu_trace(ctx, case, slot, P, mode_right):
    st = np.zeros(P.n, np.uint8)
    ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, slot, abi.fp(case["K"]), case["baseline"], mode_right, C.byref(P), abi.bp(st)))
    return st


def _intervals(case, kind):
    return (None, None) if kind == "fresh" else (case["idepth_min"], case["idepth_max"])


def _forward_and_back(ctx, oracle, case, kind, gn_mode, back):
    """L -> R on both sides; with `back`, R -> L from the oracle's forward result on both sides (test_gpu_trace_bit_exact's pattern).
    The left image is in SLOT_L, the right one in SLOT_R."""
    u, v = case["u"], case["v"]
    n = len(u)
    init_o = Ls.oracle_init(oracle, case["left"], u, v)
    init_g = tuple(np.zeros_like(a) for a in init_o)
    ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, SLOT_L, n, abi.fp(u), abi.fp(v), *[abi.fp(a) for a in init_g]))
    for a, b in zip(init_o, init_g):
        assert np.array_equal(a, b)
    imin, imax = _intervals(case, kind)
    Po, do = _points(case, init_o, imin, imax)
    Pg, dg = _points(case, init_o, imin, imax)
    so = Ls.oracle_trace(oracle, case, case["right"], Po, 1, gn_mode)
    sg = _gpu_trace(ctx, case, SLOT_R, Pg, 1)
    _same((sg, dg), (so, do))
    if not back:
        return
    good = np.nonzero(so == Ls.GOOD)[0]
    ub, vb = do["lastTraceUV"][good, 0].copy(), do["lastTraceUV"][good, 1].copy()
    inb = (ub > 6) & (vb > 6) & (ub < case["w"] - 7) & (vb < case["h"] - 7)
    ub, vb, good = ub[inb], vb[inb], good[inb]
    assert len(good) > 1000
    init_b = Ls.oracle_init(oracle, case["right"], ub, vb)
    bmin = (do["idepth_stereo"][good] * 0.1).astype(np.float32); bmax = (do["idepth_stereo"][good] * 1.9).astype(np.float32)
    Po2, do2 = abi.make_trace_points(len(ub), ub, vb, *init_b, bmin, bmax)
    Pg2, dg2 = abi.make_trace_points(len(ub), ub, vb, *init_b, bmin, bmax)
    so2 = Ls.oracle_trace(oracle, case, case["left"], Po2, 0, gn_mode)
    sg2 = _gpu_trace(ctx, case, SLOT_L, Pg2, 0)
    _same((sg2, dg2), (so2, do2))
    # the back search is as long as the forward one was far: (0.1 ... 1.9) x the disparity, clamped to maxPixSearch
    back = dict(case, u=ub, baseline=-case["baseline"])
    steps, uMin = Ls.stereo_step_count(back, bmin, bmax)
    ok = so2 == Ls.GOOD
    best = np.abs(do2["lastTraceUV"][ok, 0] - uMin[ok])
    print("back trace: status", np.bincount(so2, minlength=6), "searches of more than 64 steps:", int((steps > 64).sum()), "GOOD with best step >= 64:", int((best >= 64.5).sum()))
    assert (steps > 64).sum() > 500 and (best >= 64.5).sum() > 50


@pytest.mark.parametrize("kind", ["fresh", "finite"])
@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_trace_stereo_forward_and_back(gpu_ctx, oracle, shape, kind):
    case = Ls.stereo_case(SHAPES[shape])
    try:
        gpu_ctx.upload_pyramid(SLOT_L, [case["left"]]); gpu_ctx.upload_pyramid(SLOT_R, [case["right"]])
        _forward_and_back(gpu_ctx, oracle, case, kind, 0, back=True)
    finally:
        _release(gpu_ctx, SLOT_L, SLOT_R)


@pytest.mark.parametrize("kind", ["fresh", "finite"])
def test_trace_stereo_g2o_refinement(gpu_ctx, oracle, kind):
    """the second instantiation of the kernel (fork-live refinement), S2"""
    case = Ls.stereo_case(Ls.S2)
    try:
        gpu_ctx.upload_pyramid(SLOT_L, [case["left"]]); gpu_ctx.upload_pyramid(SLOT_R, [case["right"]])
        gpu_ctx.check(gpu_ctx.L.sdso_trace_set_gn_mode(gpu_ctx.h, 1))
        _forward_and_back(gpu_ctx, oracle, case, kind, 1, back=True)
    finally:
        gpu_ctx.L.sdso_trace_set_gn_mode(gpu_ctx.h, 0)
        _release(gpu_ctx, SLOT_L, SLOT_R)


@pytest.mark.parametrize("period", [64, 32])
def test_periodic_pair_keeps_the_earliest_of_equal_steps(gpu_ctx, oracle, period):
    """rows of period 64 px: step s + 64 has the energy of step s, bit for bit, and both are candidates of one lane.  Period 32: steps s
    and s + 32 are equal and lie on two lanes.  A merge of a lane's two candidates, or an index tie across lanes, resolved the other way
    moves every match by one period."""
    case = Ls.periodic_case(period)
    try:
        gpu_ctx.upload_pyramid(SLOT_R, [case["right"]])
        init = Ls.oracle_init(oracle, case["left"], case["u"], case["v"])
        Po, do = _points(case, init)
        Pg, dg = _points(case, init)
        so = Ls.oracle_trace(oracle, case, case["right"], Po, 1)
        sg = _gpu_trace(gpu_ctx, case, SLOT_R, Pg, 1)
        good = sg == Ls.GOOD
        disp = case["u"][good] - dg["lastTraceUV"][good, 0]
        ties = int((dg["quality"][good] == 1.0).sum())
        print("device: status", np.bincount(sg, minlength=6), "GOOD with quality == 1:", ties, "largest disparity", disp.max() if len(disp) else None)
        assert good.sum() >= 300 and ties >= 250 and (disp < Ls.MAX_PERIODIC_DISPARITY[period]).all()
        _same((sg, dg), (so, do))
    finally:
        _release(gpu_ctx, SLOT_R)


@pytest.mark.parametrize("kind", ["fresh", "finite"])
def test_prepared_trace_at_s2(gpu_ctx, oracle, kind):
    """sdso_trace_stereo_prepare / _enqueue / _fetch: two enqueues leave the result of one (the pristine copy restores the inputs)"""
    case = Ls.stereo_case(Ls.S2)
    try:
        gpu_ctx.upload_pyramid(SLOT_R, [case["right"]])
        init = Ls.oracle_init(oracle, case["left"], case["u"], case["v"])
        imin, imax = _intervals(case, kind)
        Po, do = _points(case, init, imin, imax)
        so = Ls.oracle_trace(oracle, case, case["right"], Po, 1)
        Pg, dg = _points(case, init, imin, imax)
        L, h = gpu_ctx.L, gpu_ctx.h
        gpu_ctx.check(L.sdso_trace_stereo_prepare(h, SLOT_R, abi.fp(case["K"]), case["baseline"], 1, C.byref(Pg)))
        for reps in (1, 2):
            for _ in range(reps):
                gpu_ctx.check(L.sdso_trace_stereo_enqueue(h))
            Pf, df = _points(case, init, imin, imax)
            sf = np.zeros(Pf.n, np.uint8)
            gpu_ctx.check(L.sdso_trace_stereo_fetch(h, C.byref(Pf), abi.bp(sf)))
            _same((sf, df), (so, do))
    finally:
        _release(gpu_ctx, SLOT_R)


def test_stereo_match_at_s2(gpu_ctx, oracle):
    """sdso_stereo_match_batch against the four oracle steps, as test_gpu_stereo_match_left_right_left"""
    case = Ls.stereo_case(Ls.S2)
    u, v = case["u"], case["v"]
    n = len(u)
    try:
        gpu_ctx.upload_pyramid(SLOT_L, [case["left"]]); gpu_ctx.upload_pyramid(SLOT_R, [case["right"]])
        for kind in ("fresh", "finite"):
            imin, imax = _intervals(case, kind)
            Po, do = _points(case, Ls.oracle_init(oracle, case["left"], u, v), imin, imax)
            sf = Ls.oracle_trace(oracle, case, case["right"], Po, 1)
            good = np.nonzero(sf == Ls.GOOD)[0]
            ub, vb = do["lastTraceUV"][good, 0].copy(), do["lastTraceUV"][good, 1].copy()
            Pb, db = abi.make_trace_points(len(good), ub, vb, *Ls.oracle_init(oracle, case["right"], ub, vb), None if imin is None else imin[good],
                                           None if imax is None else imax[good])
            sb = Ls.oracle_trace(oracle, case, case["left"], Pb, 0)
            M = abi.StereoMatch()
            out = dict(status_fwd=np.zeros(n, np.uint8), status_back=np.zeros(n, np.uint8), idepth_stereo=np.zeros(n, np.float32),
                       idepth_min_out=np.zeros(n, np.float32), idepth_max_out=np.zeros(n, np.float32), fwd_uv=np.zeros((n, 2), np.float32),
                       back_uv=np.zeros((n, 2), np.float32))
            M.n = n; M.u = abi.fp(u); M.v = abi.fp(v)
            if imin is not None:
                M.idepth_min_stereo = abi.fp(imin); M.idepth_max_stereo = abi.fp(imax)
                M.back_idepth_min_stereo = abi.fp(imin); M.back_idepth_max_stereo = abi.fp(imax)
            abi.bind(M, out)
            gpu_ctx.check(gpu_ctx.L.sdso_stereo_match_batch(gpu_ctx.h, SLOT_L, SLOT_R, abi.fp(case["K"]), case["baseline"], 1, C.byref(M)))
            assert np.array_equal(out["status_fwd"], sf)
            assert np.array_equal(out["idepth_stereo"][good], do["idepth_stereo"][good])
            assert np.array_equal(out["idepth_min_out"][good], do["idepth_min_stereo"][good]) and np.array_equal(out["idepth_max_out"][good], do["idepth_max_stereo"][good])
            assert np.array_equal(out["fwd_uv"], do["lastTraceUV"])
            assert (out["status_back"][sf != 0] == 255).all() and np.array_equal(out["status_back"][good], sb)
            assert np.array_equal(out["back_uv"][good], db["lastTraceUV"])
            assert len(good) > 2000 and (sb == Ls.GOOD).sum() > 1000
    finally:
        _release(gpu_ctx, SLOT_L, SLOT_R)


TRACE_ON_FIELDS = ("idepth_min_stereo", "idepth_max_stereo", "quality", "lastTraceStatus", "lastTraceUV", "lastTracePixelInterval")


def _trace_on(run, case, init, state, rows=slice(None)):
    P, d = _points(case, init, state["idepth_min"], state["idepth_max"], rows)
    d["lastTraceStatus"][:] = state["prev"][rows]
    st = np.zeros(P.n, np.uint8)
    run(abi.ip(np.ascontiguousarray(state["pg"][rows])), P, st)
    return st, d


def _oracle_trace_on(oracle, case):
    def run(pg, P, st):
        assert oracle.orc_trace_on_batch(abi.fp(case["new"]), case["w"], case["h"], 2, case["geoms"], pg, C.byref(P), abi.bp(st)) == 0
    return run


def _gpu_trace_on(ctx, case):
    def run(pg, P, st):
        ctx.check(ctx.L.sdso_trace_on_batch(ctx.h, SLOT_NEW, 2, case["geoms"], pg, C.byref(P), abi.bp(st)))
    return run


def trace_on_oracle_result(oracle, case):
    """the oracle's trace of the mixed-state batch, with the conditions the batch must meet"""
    init = Ls.oracle_init(oracle, case["host"], case["u"], case["v"])
    state = Ls.trace_on_mixed_state(case)
    so, do = _trace_on(_oracle_trace_on(oracle, case), case, init, state)
    assert {Ls.GOOD, Ls.OOB, Ls.OUTLIER, Ls.SKIPPED}.issubset(set(np.unique(so)))
    # finite intervals of the first geometry: matches in the second pass; searches of more than 64 steps, clamped and not
    uMin, vMin, dist = Ls.trace_on_interval_ends(case, state["idepth_min"], state["idepth_max"])
    fin = state["long_interval"] & (state["pg"] == 0)
    far = fin & (so == Ls.GOOD) & (np.hypot(do["lastTraceUV"][:, 0] - uMin, do["lastTraceUV"][:, 1] - vMin) >= 64.5)
    searched = fin & ((so == Ls.GOOD) | (so == Ls.OUTLIER))
    mps = Ls.max_pix_search(case["w"], case["h"])
    clamped, unclamped = searched & (dist > mps + 0.5), searched & (dist >= 63.5) & (dist < mps - 0.5)
    print("traceOn %dx%d: status" % (case["w"], case["h"]), np.bincount(so, minlength=6), "finite-interval GOOD at >= 64.5 px from uMin:", int(far.sum()),
          "searched finite intervals of more than 64 steps, clamped / not:", int(clamped.sum()), int(unclamped.sum()))
    assert far.sum() >= 50
    assert clamped.sum() >= 20 and unclamped.sum() >= 20
    return init, state, (so, do)


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_trace_on_mixed_prior_states(gpu_ctx, oracle, shape):
    case = Ls.trace_on_case(SHAPES[shape])
    init, state, want = trace_on_oracle_result(oracle, case)
    try:
        gpu_ctx.upload_pyramid(SLOT_NEW, [case["new"]])
        _same(_trace_on(_gpu_trace_on(gpu_ctx, case), case, init, state), want, TRACE_ON_FIELDS)
    finally:
        _release(gpu_ctx, SLOT_NEW)


def _earliest_of_equal_steps(name, period, u, status, uv, quality):
    """the device's own result on a periodic pair: enough exact ties, every match at the earliest of the equal steps"""
    good = status == Ls.GOOD
    disp = u[good] - uv[good, 0]
    ties = int((quality[good] == 1.0).sum())
    print(name, "period", period, "device: status", np.bincount(status, minlength=6), "GOOD with quality == 1:", ties, "largest disparity", disp.max() if len(disp) else None)
    assert good.sum() >= 300 and ties >= 250 and (disp < Ls.MAX_PERIODIC_DISPARITY[period]).all()


@pytest.mark.parametrize("period", [64, 32])
def test_trace_on_periodic_pair_keeps_the_earliest_of_equal_steps(gpu_ctx, oracle, period):
    """the periodic pair through trace_on_point, which has step loops, a merge of a lane's two candidates and an index rule of its own:
    sdso_trace_on_batch (k_trace_on) and sdso_imm_add_frame + the key form of sdso_imm_trace (k_imm_trace_on)"""
    ctx, L = gpu_ctx, gpu_ctx.L
    case = Ls.periodic_trace_on_case(period)
    n = len(case["u"])
    fresh = dict(idepth_min=None, idepth_max=None, prev=np.full(n, Ls.UNINITIALIZED, np.uint8), pg=np.zeros(n, np.int32))
    try:
        ctx.upload_pyramid(SLOT_NEW, [case["new"]]); ctx.upload_pyramid(SLOT_HOST, [case["host"]])
        init = Ls.oracle_init(oracle, case["host"], case["u"], case["v"])

        def gpu(pg, P, st):
            ctx.check(L.sdso_trace_on_batch(ctx.h, SLOT_NEW, 1, case["geoms"], pg, C.byref(P), abi.bp(st)))

        def orc(pg, P, st):
            assert oracle.orc_trace_on_batch(abi.fp(case["new"]), case["w"], case["h"], 1, case["geoms"], pg, C.byref(P), abi.bp(st)) == 0
        sg, dg = _trace_on(gpu, case, init, fresh)
        _earliest_of_equal_steps("sdso_trace_on_batch", period, case["u"], sg, dg["lastTraceUV"], dg["quality"])
        _same((sg, dg), _trace_on(orc, case, init, fresh), TRACE_ON_FIELDS)

        m = C.c_int(-1)
        ctx.check(L.sdso_imm_add_frame(ctx.h, PERIODIC_HOST_ID, SLOT_HOST, abi.fp(case["map"]), C.byref(m)))
        ref = R.add_frame(oracle, case["host"], case["map"])
        assert m.value == len(ref["u"]) == Ls.PERIODIC_RESIDENT_POINTS
        c = np.full(abi.IMM_NCOUNTS, -1, np.int32)
        ctx.check(L.sdso_imm_trace(ctx.h, SLOT_NEW, -1, 1, _imm_geoms(PERIODIC_HOST_ID, case["geom"]), abi.fp(case["K4"]), abi.fp(case["Ki"]), case["baseline"], abi.ip(c)))
        cr, _, _ = R.trace(oracle, [(ref, case["geom"])], case["new"], None, case["K4"], case["Ki"], case["baseline"])
        got = ctx.imm_get(PERIODIC_HOST_ID)
        _earliest_of_equal_steps("sdso_imm_trace", period, got["u"], got["lastTraceStatus"], got["lastTraceUV"], got["quality"])
        assert np.array_equal(c, cr)
        assert R.same(got, ref) is None, R.same(got, ref)
    finally:
        L.sdso_imm_release_host(ctx.h, PERIODIC_HOST_ID)
        _release(ctx, SLOT_NEW, SLOT_HOST)


def test_partial_workgroups(gpu_ctx, oracle):
    """the first 1, 15, 17 points (traceStereo: 16 per workgroup) and 1, 3, 5 points (traceOn: 4 per workgroup) of the S2 fresh batches
    equal the same rows of the full run.  The first rows of the traceOn batch lie at the upper border and leave the image, so the same
    counts are also taken from the first run of five points whose matches all lie in the second pass."""
    case = Ls.stereo_case(Ls.S2)
    on = Ls.trace_on_case(Ls.S2)
    try:
        gpu_ctx.upload_pyramid(SLOT_R, [case["right"]]); gpu_ctx.upload_pyramid(SLOT_NEW, [on["new"]])
        init = Ls.oracle_init(oracle, case["left"], case["u"], case["v"])
        P, d = _points(case, init)
        full = _gpu_trace(gpu_ctx, case, SLOT_R, P, 1), d
        assert (full[0][:17] == Ls.GOOD).sum() >= 10
        for n in (1, 15, 17):
            P, d = _points(case, init, rows=slice(0, n))
            _same((_gpu_trace(gpu_ctx, case, SLOT_R, P, 1), d), _rows(full, slice(0, n)))
        init = Ls.oracle_init(oracle, on["host"], on["u"], on["v"])
        fresh = dict(idepth_min=None, idepth_max=None, prev=np.full(len(on["u"]), Ls.UNINITIALIZED, np.uint8), pg=np.zeros(len(on["u"]), np.int32))
        run = _gpu_trace_on(gpu_ctx, on)
        full = _trace_on(run, on, init, fresh)
        u0, v0 = Ls.project0(on["KRKi"], on["u"], on["v"])
        far = (full[0] == Ls.GOOD) & (np.hypot(full[1]["lastTraceUV"][:, 0] - u0, full[1]["lastTraceUV"][:, 1] - v0) >= 64.5)
        runs = np.nonzero(np.convolve(far, np.ones(5, int), "valid") == 5)[0]
        assert len(runs) > 0
        for k0 in (0, int(runs[0])):
            for n in (1, 3, 5):
                _same(_trace_on(run, on, init, fresh, slice(k0, k0 + n)), _rows(full, slice(k0, k0 + n)), TRACE_ON_FIELDS)
    finally:
        _release(gpu_ctx, SLOT_R, SLOT_NEW)


def _imm_geoms(host_id, g):
    G = (abi.ImmGeom * 1)()
    G[0].host_id = host_id
    for k in ("KRKi", "Kt", "aff", "KRi", "t"):
        getattr(G[0], k)[:] = [float(x) for x in g[k]]
    return G


def test_resident_set_at_s2(gpu_ctx, oracle):
    """sdso_imm_add_frame + sdso_imm_trace (k_imm_trace_on and the stereo chain behind it) in the key form and in the non-key form with
    both refinement modes, each on a host of its own added from the same map, against immature_ref"""
    ctx, L = gpu_ctx, gpu_ctx.L
    case = Ls.resident_case()
    try:
        ctx.upload_pyramid(SLOT_HOST, [case["host"]]); ctx.upload_pyramid(SLOT_FL, [case["left"]]); ctx.upload_pyramid(SLOT_FR, [case["right"]])
        key_hist = None
        for hid, (nonkey, gn) in zip(HOST_IDS, ((False, 0), (True, 0), (True, 1))):
            n = C.c_int(-1)
            ctx.check(L.sdso_imm_add_frame(ctx.h, hid, SLOT_HOST, abi.fp(case["map"]), C.byref(n)))
            ref = R.add_frame(oracle, case["host"], case["map"])
            assert n.value == len(ref["u"]) == Ls.RESIDENT_POINTS and n.value % 4 != 0
            assert R.same(ctx.imm_get(hid), ref) is None, R.same(ctx.imm_get(hid), ref)
            c = np.full(abi.IMM_NCOUNTS, -1, np.int32)
            ctx.check(L.sdso_trace_set_gn_mode(ctx.h, gn))
            ctx.check(L.sdso_imm_trace(ctx.h, SLOT_FL, SLOT_FR if nonkey else -1, 1, _imm_geoms(hid, case["geom"]), abi.fp(case["K4"]), abi.fp(case["Ki"]),
                                       case["baseline"], abi.ip(c)))
            ctx.check(L.sdso_trace_set_gn_mode(ctx.h, 0))
            u0, v0 = Ls.project0(case["geom"]["KRKi"], ref["u"], ref["v"])
            cr, on_hist, fwd_hist = R.trace(oracle, [(ref, case["geom"])], case["left"], case["right"] if nonkey else None, case["K4"], case["Ki"], case["baseline"], gn)
            print("nonkey", nonkey, "gn", gn, "counts", c, "statement", cr, "traceOn", on_hist, "forward traceStereo", fwd_hist)
            assert np.array_equal(c, cr)
            got = ctx.imm_get(hid)
            assert R.same(got, ref) is None, R.same(got, ref)
            if not nonkey:       # the statement's traceOn result, before any stereo step touches it
                good = ref["lastTraceStatus"] == Ls.GOOD
                far = np.hypot(ref["lastTraceUV"][good, 0] - u0[good], ref["lastTraceUV"][good, 1] - v0[good])
                assert on_hist[Ls.GOOD] == good.sum() > 500 and (far >= 64.5).mean() >= 0.25
                key_hist = on_hist
            else:                # the same traceOn step on the same points, then the stereo chain
                assert np.array_equal(on_hist, key_hist) and cr[R.C_UPDATED] > 50
    finally:
        L.sdso_trace_set_gn_mode(ctx.h, 0)
        for hid in HOST_IDS:
            L.sdso_imm_release_host(ctx.h, hid)
        _release(ctx, SLOT_HOST, SLOT_FL, SLOT_FR)
