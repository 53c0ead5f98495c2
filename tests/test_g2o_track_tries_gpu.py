"""sdso_g2o_track_newest_coarse_batch and sdso_g2o_track_new_coarse — the fork-live coarse tracker resident on the device (k_g2o_track_lm:
one launch, one workgroup per try) and the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511) around it — on the GPU,
through the C-ABI.

The problem is the tries tests' own (synth.tracker_problem(w=640, h=480, npts=2000, seed=2001): 4 levels, pc_n = [9632, 8396, 5614, 2308],
none a multiple of the 512-lane workgroup).  What the CPU oracle (orc_g2o_track_newest_coarse) gives on it: G is good with 46 evaluations
and residuals 4.120725 / 3.669631 / 3.639926 / 3.514573; H is not good with 47 evaluations and 8.839475 / 10.037558 / 11.066720 / 11.917776;
under G's bounds H aborts on level 3 (11.917776 against 1.5 * 3.514573, a margin of 126 %); the list [0, 2 truth, truth / 2, truth] moves
the winner 0 -> 1 -> 2 -> 3 on relative gaps of 1.4e-3, 1.9e-4 and 5.4e-6.

Bars (the project's own for the fork-live tracker, tests/test_g2o_factors.py::test_gpu_g2o_tracker_matches_oracle): pose 1e-9, a 1e-9,
b 1e-7, residuals and achievedRes 1e-6 relative (they pass through sqrtf), flow indicators bit-equal, integers equal.  Bit-equality
between the new route and the host-driven call is not asked: the order of the sums and the device's pow differ."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth
import track_tries_cases as cases
import track_tries_ref as ref
import g2o_track_tries_cases as g2o

pytestmark = pytest.mark.gpu

AFF0 = (0.0, 0.0)
STARTS = {"I": np.zeros(6), "G": cases.G, "2T": 2 * cases.TRUTH, "T/2": cases.TRUTH / 2, "T": cases.TRUTH, "H": cases.H}
LISTS = {"HHG": ([cases.H, cases.H, cases.G], AFF0, 1e9), "GHH": ([cases.G, cases.H, cases.H], AFF0, 0.0), "HH": ([cases.H, cases.H], (0.03, -1.5), 1e9),
         "GH": ([cases.G, cases.H], AFF0, 1e9), "ties": ([np.zeros(6), 2 * cases.TRUTH, cases.TRUTH / 2, cases.TRUTH], AFF0, 0.0)}


@pytest.fixture(scope="module")
def prob():
    return cases.problem()


@pytest.fixture(scope="module")
def start_poses():
    return {k: cases.poses([x])[0] for k, x in STARTS.items()}


@pytest.fixture(scope="module")
def oracle_singles(oracle, prob, start_poses):
    """the oracle's fork-live trackNewestCoarse from every start under NaN bounds, once"""
    prm = helpers.track_params(prob)
    return {k: g2o.oracle_single(oracle, prob, prm, p, AFF0) for k, p in start_poses.items()}


@pytest.fixture(scope="module")
def oracle_loops(oracle, prob):
    """the reference's loop over the oracle's fork-live trackNewestCoarse for every list, once"""
    prm = helpers.track_params(prob)
    return {k: g2o.oracle_loop(oracle, prob, prm, cases.poses(xs), a0, [rm] * 5) for k, (xs, a0, rm) in LISTS.items()}


@pytest.fixture()
def ctx(gpu_ctx, prob):
    gpu_ctx.upload_pyramid(cases.NEW_SLOT, prob["pyr_new"])
    gpu_ctx.set_ref(cases.REF_SLOT, prob["pc"])
    return gpu_ctx


def _same_bits(a, b):
    return len(a) == len(b) and all(ref.same_double(x, y) for x, y in zip(a, b))


def _one(ctx, prm, pose, aff0=AFF0, **kw):
    rc, T, A, O = g2o.batch(ctx, [prm], [pose], [aff0], **kw)
    ctx.check(rc)
    return cases.se3_tuple(T[0]), (A[0].a, A[0].b), O[0]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_batch_of_one_against_oracle_and_host_call(ctx, prob, start_poses, oracle_singles):
    """identity, G, 2 truth, truth / 2, truth: the oracle and sdso_g2o_track_newest_coarse on the same slots; H: integers, verdict and
    residuals only (a near-singular system); the abort path leaves the references untouched"""
    prm = helpers.track_params(prob)
    assert [len(p["u"]) for p in prob["pc"]] == [9632, 8396, 5614, 2308]
    assert g2o.ints_of(oracle_singles["G"][2])[:3] == (1, [2, 2, 2, 2, 0], 46) and g2o.ints_of(oracle_singles["H"][2])[:3] == (0, [2, 2, 2, 2, 0], 47)
    for k in ("I", "G", "2T", "T/2", "T", "H"):
        po, ao, oo = oracle_singles[k]
        rc, ph, ah, oh = g2o.host_single(ctx, prm, start_poses[k], AFF0)
        ctx.check(rc)
        pn, an, on = _one(ctx, prm, start_poses[k])
        print(k, "ints", g2o.ints_of(on), "residuals", list(on.lastResiduals)[:4], "oracle", list(oo.lastResiduals)[:4], "host call", list(oh.lastResiduals)[:4],
              "|pose - oracle|", np.abs(np.array(pn) - np.array(po)).max(), "|pose - host call|", np.abs(np.array(pn) - np.array(ph)).max(),
              "aff", an, ao, ah)
        assert g2o.ints_of(on) == g2o.ints_of(oo) == g2o.ints_of(oh), k
        assert g2o.res_close(on.lastResiduals, oo.lastResiduals) and g2o.res_close(on.lastResiduals, oh.lastResiduals), k
        if k == "H":
            continue
        assert on.good == 1, k
        assert g2o.estimate_close(pn, an, po, ao) and g2o.estimate_close(pn, an, ph, ah), k
        assert _same_bits(list(on.lastFlowIndicators), list(oo.lastFlowIndicators)) and _same_bits(list(on.lastFlowIndicators), list(oh.lastFlowIndicators)), k
    # the abort path: minResForAbort = 0.01 ends the call on the coarsest level, the references stay as they came
    for i in range(5):
        prm.minResForAbort[i] = 0.01
    rc, ph, ah, oh = g2o.host_single(ctx, prm, start_poses["G"], (0.02, -0.7))
    ctx.check(rc)
    pn, an, on = _one(ctx, prm, start_poses["G"], (0.02, -0.7))
    assert on.good == 0 and g2o.ints_of(on) == g2o.ints_of(oh) and on.iterations[3] == 2 and list(on.iterations)[:3] == [0, 0, 0]
    assert pn == start_poses["G"] and an == (0.02, -0.7)
    assert g2o.res_close(on.lastResiduals, oh.lastResiduals) and np.isfinite(on.lastResiduals[3]) and all(np.isnan(on.lastResiduals[l]) for l in (0, 1, 2, 4))


# ---------------------------------------------------------------------------------------------------------------- 2
def test_batch_composition(ctx, prob, start_poses):
    """the six starts one by one, as a batch of 6, and inside a batch of 53 padded with copies of H: every try's pose, affine pair,
    result and trace bit-equal; twice the same call gives the same bytes"""
    prm = helpers.track_params(prob)
    keys = ["I", "G", "2T", "T/2", "T", "H"]
    six = [start_poses[k] for k in keys]
    singles = [g2o.batch(ctx, [prm], [p], [AFF0]) for p in six]
    for rc, _, _, _ in singles:
        ctx.check(rc)
    for poses in (six, six + [start_poses["H"]] * 47):
        n = len(poses)
        runs = []
        for _ in range(2):
            rc, T, A, O = g2o.batch(ctx, [prm] * n, poses, [AFF0] * n)
            ctx.check(rc)
            runs.append((bytes(T), bytes(A), bytes(O)))
        assert runs[0] == runs[1], n
        for k in range(6):
            _, T1, A1, O1 = singles[k]
            assert bytes(T[k]) == bytes(T1[0]) and bytes(A[k]) == bytes(A1[0]) and bytes(O[k]) == bytes(O1[0]), (n, keys[k])
        for k in range(6, n):
            assert bytes(O[k]) == bytes(O[5]) and bytes(T[k]) == bytes(T[5]), (n, k)
    # the traces, through the records of sdso_g2o_track_new_coarse: try 0 = H is not good, so phase 2 runs tries 1.. under NaN bounds
    # as ONE batch — of one, of 6, of 52
    H = start_poses["H"]
    alone = []
    for p in six:
        rc, _, _, R = g2o.new_coarse(ctx, prm, [H, p], AFF0, [0.0] * 5)
        ctx.check(rc)
        alone.append(g2o.in_members(R[1]))
    for tries in ([H] + six, [H] + six + [H] * 46):
        got = []
        for _ in range(2):
            rc, out, rmse, R = g2o.new_coarse(ctx, prm, tries, AFF0, [0.0] * 5)
            ctx.check(rc)
            got.append((bytes(out), bytes(R)))
        assert got[0] == got[1], len(tries)
        assert R[0].end_good == 0 and out.tryIterations == len(tries)
        for k in range(6):
            assert g2o.in_members(R[1 + k]) == alone[k], (len(tries), keys[k])
            assert R[1 + k].trace.n == 4 and [R[1 + k].trace.lvl[e] for e in range(4)] == [3, 2, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- 3
def _g2o_eval(L, prm, lvl, T_cull, T_vertex, aff_vertex):
    base = abi.TrackEval()
    Tc = abi.SE3.from_Rt(*T_cull)
    a = abi.Aff(*aff_vertex)
    L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(Tc), C.byref(a), 1.0, C.byref(base))
    ev = abi.G2oTrackEval()
    ev.lvl, ev.w, ev.h = lvl, base.w, base.h
    ev.fx, ev.fy, ev.cx, ev.cy = base.fx, base.fy, base.cx, base.cy
    ev.Ki[:] = base.Ki[:]; ev.RKi[:] = base.RKi[:]; ev.t_cull[:] = base.t[:]
    ev.R[:] = np.asarray(T_vertex[0], np.float64).ravel().tolist(); ev.t[:] = np.asarray(T_vertex[1], np.float64).tolist()
    ev.ab[:] = base.affLL[:]
    ev.b0 = prm.ref_aff_g2l.b
    ev.cutoffTH, ev.huberTH = base.cutoffTH, base.huberTH
    return ev


def test_stored_edge_sets_survive(ctx, prob, start_poses):
    """sdso_g2o_track_add_edges + _linearize, then the new batch on the same slots, then _linearize again: H, b, chi2 bit-equal"""
    prm = helpers.track_params(prob)
    T0 = synth.se3_exp(np.array([0.4, -0.1, 1.5, 0.01, 0.25, -0.01]))     # the cull pose of test_gpu_track_edges_bit_exact: part of the template leaves the image
    Tv = synth.se3_exp(cases.G)
    sets = {}
    for lvl in (0, 2):
        ev = _g2o_eval(ctx.L, prm, lvl, T0, Tv, (0.015, 1.0))
        res = np.zeros(6); ne = C.c_int(0)
        ctx.check(ctx.L.sdso_g2o_track_add_edges(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(ev), abi.dp(res), C.byref(ne), None, None))
        assert 0 < ne.value < len(prob["pc"][lvl]["u"])

        def lin(ev=ev):
            H = np.zeros(64); b = np.zeros(8); chi = np.zeros(2)
            ctx.check(ctx.L.sdso_g2o_track_linearize(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(chi), None, None))
            return H.tobytes() + b.tobytes() + chi.tobytes()
        sets[lvl] = (lin, lin())
    poses = [start_poses[k] for k in ("I", "G", "H")]
    rc, T, A, O = g2o.batch(ctx, [prm] * 3, poses, [AFF0] * 3)
    ctx.check(rc)
    assert [O[k].good for k in range(3)] == [1, 1, 0]
    for lvl, (lin, before) in sets.items():
        assert lin() == before, lvl


# ---------------------------------------------------------------------------------------------------------------- 4
def _run(ctx, prob, name):
    xs, aff0, rm = LISTS[name]
    tries = cases.poses(xs)
    rc, out, rmse, R = g2o.new_coarse(ctx, helpers.track_params(prob), tries, aff0, [rm] * 5)
    ctx.check(rc)
    # for every list: the outputs are the rules applied to the returned `in` members, bit for bit, by sdso_track_tries_replay and by the
    # Python loop; a trace has at most five events, levels strictly descending
    n = len(tries)
    R2 = (abi.TrackTry * n)()
    for k in range(n):
        R2[k].trace = R[k].trace; R2[k].end_good = R[k].end_good; R2[k].end_pose = R[k].end_pose; R2[k].end_aff = R[k].end_aff
    T = (abi.SE3 * n)(*[cases.se3_of(t) for t in tries])
    ran = [R[k].ran for k in range(n)]
    rc2, out2, rmse2 = cases.replay(ctx.L, R2, T, aff0, [rm] * 5, 1.5)
    assert rc2 == 0
    assert bytes(out2) == bytes(out) and _same_bits(rmse2, rmse), name
    want = ref.track_new_coarse(cases.from_c(R), tries, aff0, [rm] * 5, 1.5)
    for k in range(n):
        if ran[k]:
            assert bytes(R2[k]) == bytes(R[k]), (name, k)
        else:
            assert R2[k].ran == 0 and want["seen"][k] is None and bytes(R[k]) == bytes(abi.TrackTry()), (name, k)   # (a try after the stop: zeroed)
    cases.assert_equal_to_ref(out, rmse, R, want, name)
    for k in range(n):
        lv = [R[k].trace.lvl[e] for e in range(R[k].trace.n)]
        assert len(lv) <= 5 and all(a > b for a, b in zip(lv, lv[1:])), (name, k, lv)
    return tries, out, rmse, R


def _loop_close(out, rmse, want):
    """pose / affine / achievedRes within the bars of the oracle loop"""
    assert g2o.estimate_close(cases.se3_tuple(out.pose), (out.aff.a, out.aff.b), want["pose"], want["aff"])
    assert g2o.res_close(out.achievedRes[:], want["achievedRes"]) and _same_bits(rmse, out.achievedRes[:])


def test_loop_hopeless_tries_first(ctx, prob, oracle_loops):
    """[H, H, G], lastCoarseRMSE = 1e9"""
    want = oracle_loops["HHG"]
    assert (want["winner"], want["tryIterations"], want["haveOneGood"]) == (2, 3, 1)
    tries, out, rmse, R = _run(ctx, prob, "HHG")
    print("achievedRes", out.achievedRes[:], "oracle", want["achievedRes"])
    assert (out.winner, out.tryIterations, out.haveOneGood) == (2, 3, 1)
    assert [R[k].ran for k in range(3)] == [1, 1, 1] and [R[k].good for k in range(3)] == [s["good"] for s in want["seen"]] == [0, 0, 1]
    _loop_close(out, rmse, want)


def test_loop_good_try_first_aborts_the_hopeless_ones(ctx, prob, oracle_loops):
    """[G, H, H], lastCoarseRMSE = 0 (never stops): both H abort on level 3 under G's bounds"""
    want = oracle_loops["GHH"]
    assert (want["winner"], want["tryIterations"]) == (0, 3) and [s["abort_lvl"] for s in want["seen"]] == [-1, 3, 3]
    tries, out, rmse, R = _run(ctx, prob, "GHH")
    assert (out.winner, out.tryIterations, out.haveOneGood) == (0, 3, 1)
    for k in (1, 2):
        print("H under G's bounds: level 3 at", R[k].lastResiduals[3], "against 1.5 *", out.achievedRes[3])
        assert (R[k].ran, R[k].good, R[k].abort_lvl, R[k].winner) == (1, 0, 3, 0)
        assert all(np.isnan(R[k].lastResiduals[l]) for l in (0, 1, 2)) and np.isfinite(R[k].lastResiduals[3])
        assert R[k].trace.n == 1                                       # it ran under G's bounds: the abort ended it on the device
        assert bytes(R[k].pose) == bytes(cases.se3_of(tries[k])) and (R[k].aff.a, R[k].aff.b) == AFF0
    _loop_close(out, rmse, want)


def test_loop_no_good_try(ctx, prob, oracle_loops):
    """[H, H] from a non-zero aff_last_2_l: the ending of FullSystem.cpp:503-508"""
    want = oracle_loops["HH"]
    assert want["haveOneGood"] == 0
    tries, out, rmse, R = _run(ctx, prob, "HH")
    assert (out.haveOneGood, out.winner, out.tryIterations) == (0, -1, 2)
    assert bytes(out.pose) == bytes(cases.se3_of(tries[0])) and (out.aff.a, out.aff.b) == LISTS["HH"][1]
    assert out.flowVecs[:] == [0.0, 0.0, 0.0]
    assert all(np.isnan(x) for x in out.achievedRes[:]) and all(np.isnan(x) for x in rmse)


def test_loop_stops_after_phase_one(ctx, prob, start_poses):
    """[G, H] with lastCoarseRMSE = 1e9: the loop stops at try 0, try 1 never runs, the outputs are the batch-of-one run of G"""
    prm = helpers.track_params(prob)
    pn, an, on = _one(ctx, prm, start_poses["G"])
    tries, out, rmse, R = _run(ctx, prob, "GH")
    assert (out.haveOneGood, out.winner, out.tryIterations) == (1, 0, 1)
    assert R[1].ran == 0 and bytes(R[1]) == bytes(abi.TrackTry())
    assert cases.se3_tuple(out.pose) == pn and (out.aff.a, out.aff.b) == an
    assert _same_bits(out.achievedRes[:], list(on.lastResiduals)) and _same_bits(rmse, list(on.lastResiduals))
    assert _same_bits(out.flowVecs[:], list(on.lastFlowIndicators)) and _same_bits(R[0].lastResiduals[:], list(on.lastResiduals))
    # without records: the same result
    rc, out2, rmse2, _ = g2o.new_coarse(ctx, prm, tries, AFF0, [1e9] * 5, with_recs=False)
    ctx.check(rc)
    assert bytes(out2) == bytes(out) and _same_bits(rmse2, rmse)


def test_loop_ties(ctx, prob, oracle_loops):
    """[0, 2 truth, truth / 2, truth], lastCoarseRMSE = 0: the oracle's successive winners are further apart than twice the residual bar,
    so the oracle's winner is demanded"""
    want = oracle_loops["ties"]
    r0 = [s["lastResiduals"][0] for s in want["seen"]]
    print("oracle level-0 residuals", r0, "winner", want["winner"])
    assert want["winner"] == 3 and all(s["winner"] for s in want["seen"])
    for a, b in zip(r0, r0[1:]):
        assert a > b and (a - b) > 2 * g2o.RES_RTOL * a               # (5.4e-6 relative at the closest)
    tries, out, rmse, R = _run(ctx, prob, "ties")
    print("level-0 residuals", [R[k].lastResiduals[0] for k in range(4)], "winner", out.winner)
    assert (out.winner, out.tryIterations, out.haveOneGood) == (3, 4, 1) and all(R[k].ran == 1 for k in range(4))
    _loop_close(out, rmse, want)


# ---------------------------------------------------------------------------------------------------------------- 5
SHAPES = {"sub-wave coarsest": [300, 257, 64, 1], "empty coarsest": [1, 63, 65, 0], "empty middle": [700, 65, 0, 63], "empty": [0, 0, 0, 0]}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_smallest_shapes(gpu_ctx, prob, start_poses, shape):
    """templates cut from the same pc: a level below one wave, one over a wave, an empty middle level, an empty coarsest level, nothing at
    all.  The batch of {identity, G, H} against sdso_g2o_track_newest_coarse on the same slots."""
    counts = SHAPES[shape]
    ctx = gpu_ctx
    ctx.upload_pyramid(cases.NEW_SLOT, prob["pyr_new"])
    pc = [{k: np.ascontiguousarray(p[k][:m]) for k in ("u", "v", "idepth", "color")} for p, m in zip(prob["pc"], counts)]
    ctx.set_ref(17, pc)
    prm = helpers.track_params(prob)
    keys = ("I", "G", "H")
    poses = [start_poses[k] for k in keys]
    rc, T, A, O = g2o.batch(ctx, [prm] * 3, poses, [AFF0] * 3, ref_slot=17)
    assert rc == 0
    for k, key in enumerate(keys):
        rch, ph, ah, oh = g2o.host_single(ctx, prm, poses[k], AFF0, ref_slot=17)
        ctx.check(rch)
        pn, an, on = cases.se3_tuple(T[k]), (A[k].a, A[k].b), O[k]
        print(shape, key, "ints", g2o.ints_of(on), "host call", g2o.ints_of(oh), "residuals", list(on.lastResiduals), list(oh.lastResiduals),
              "|pose - host call|", np.abs(np.array(pn) - np.array(ph)).max(), "aff", an, ah)
        assert g2o.ints_of(on) == g2o.ints_of(oh), (shape, key)
        assert g2o.res_close(on.lastResiduals, oh.lastResiduals), (shape, key)
        assert g2o.estimate_close(pn, an, ph, ah), (shape, key)
        assert _same_bits(list(on.lastFlowIndicators), list(oh.lastFlowIndicators)), (shape, key)
    if shape == "empty":
        assert g2o.ints_of(O[0]) == (1, [1, 1, 1, 1, 0], 20, 0) and all(np.isnan(x) for x in O[0].lastResiduals)
    ctx.check(ctx.L.sdso_track_release_ref(ctx.h, 17))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_refusals_leave_everything_unchanged(ctx, prob):
    """Every refusal comes before any device work and writes nothing; the same good call before and after gives the same bytes.
    prm.minResForAbort is ignored."""
    ERR_ARG = -1
    L, h = ctx.L, ctx.h
    prm = helpers.track_params(prob)
    top = prm.coarsestLvl
    ctx.upload_pyramid(5, prob["pyr_new"][:top])                  # the same image without the level the call starts on
    tries = cases.poses([cases.G, cases.H])

    def good_call(p=prm):
        rc, out, rmse, R = g2o.new_coarse(ctx, p, tries, AFF0, [0.0] * 5)
        ctx.check(rc)
        return bytes(out), bytes(R), rmse

    before = good_call()
    n = len(tries)
    T = (abi.SE3 * n)(*[cases.se3_of(t) for t in tries])
    a = abi.Aff(*AFF0)

    def refused(ref_slot=cases.REF_SLOT, new_slot=cases.NEW_SLOT, p=prm, ntries=n, T=T, a=C.byref(a), rm=True, out=True):
        o = abi.TrackTriesResult(); o.winner = 77
        R = (abi.TrackTry * n)(); R[0].ran = 55
        was = bytes(R)
        m = (C.c_double * 5)(1.0, 2.0, 3.0, 4.0, 5.0)
        rc = L.sdso_g2o_track_new_coarse(h, ref_slot, new_slot, C.byref(p) if p is not None else None, ntries, T, a, m if rm else None, 1.5,
                                         C.byref(o) if out else None, R)
        assert rc == ERR_ARG
        assert o.winner == 77 and bytes(R) == was and list(m) == [1.0, 2.0, 3.0, 4.0, 5.0]

    refused(p=None); refused(T=None); refused(a=None); refused(rm=False); refused(out=False)
    refused(ntries=0); refused(ntries=-1); refused(ntries=65)
    refused(ref_slot=999); refused(new_slot=998)
    refused(new_slot=5)                                           # lacks the start level
    bad = helpers.track_params(prob); bad.coarsestLvl = 7
    refused(p=bad)
    off = helpers.track_params(prob); off.w[1] += 1
    refused(p=off)
    assert L.sdso_g2o_track_new_coarse(None, 1, 2, C.byref(prm), n, T, C.byref(a), (C.c_double * 5)(), 1.5, C.byref(abi.TrackTriesResult()), None) != 0
    # the batch entry refuses the same way, with its outputs untouched
    P = (abi.TrackParams * 1)(abi.TrackParams.from_buffer_copy(bytes(prm))); O = (abi.TrackResult * 1)(); O[0].evaluations = 91
    one = (C.c_int * 1)(cases.REF_SLOT); two = (C.c_int * 1)(cases.NEW_SLOT); five = (C.c_int * 1)(5); T1 = (abi.SE3 * 1)(cases.se3_of(tries[0])); A1 = (abi.Aff * 1)()
    was = bytes(T1)
    assert L.sdso_g2o_track_newest_coarse_batch(h, 0, one, two, P, T1, A1, O) == ERR_ARG
    assert L.sdso_g2o_track_newest_coarse_batch(h, 1, one, five, P, T1, A1, O) == ERR_ARG
    assert L.sdso_g2o_track_newest_coarse_batch(h, 1, None, two, P, T1, A1, O) == ERR_ARG
    assert O[0].evaluations == 91 and bytes(T1) == was
    after = good_call()
    assert before[0] == after[0] and before[1] == after[1] and _same_bits(before[2], after[2])
    p2 = helpers.track_params(prob)
    for i in range(5):
        p2.minResForAbort[i] = 0.01
    ignored = good_call(p2)
    assert before[0] == ignored[0] and before[1] == ignored[1] and _same_bits(before[2], ignored[2])
