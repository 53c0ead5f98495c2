"""sdso_track_new_coarse — the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511) — on the GPU, through the C-ABI.

One small problem (synth.tracker_problem(w=640, h=480, npts=2000, seed=2001): one template, one frame, 4 levels) and two starts:
G converges (oracle residuals 6.37580 / 5.07021 / 4.32762 / 3.50754), H is hopeless (11.79 / 11.50 / 10.89 / 9.49, not good; under G's
bounds it aborts on level 3 at 9.49 against 1.5 * 3.5075 = 5.26, a margin of 80 %).  Where the oracle's margins are that large the
oracle's winner index is demanded; where converging tries tie (their level-0 residuals differ by 1e-6 relative, below what the order of
a float sum moves) the call is held to the loop's rules on its own per-try numbers, and to the oracle within the tie.

Tolerances: pose 1e-5, affine 1e-5 / 1e-3 (tests/test_tracker_gpu.py); achievedRes 1e-5 relative (the order-of-summation bound of the
cluster test)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import track_tries_cases as cases
import track_tries_ref as ref

pytestmark = pytest.mark.gpu

AFF0 = (0.0, 0.0)
LISTS = {"HHG": ([cases.H, cases.H, cases.G], 1e9), "GHH": ([cases.G, cases.H, cases.H], 0.0), "HH": ([cases.H, cases.H], 1e9),
         "ties": ([np.zeros(6), 2 * cases.TRUTH, cases.TRUTH / 2, cases.TRUTH], 0.0)}


@pytest.fixture(scope="module")
def prob():
    return cases.problem()


@pytest.fixture(scope="module")
def oracle_loops(oracle, prob):
    """the reference's loop over the oracle's trackNewestCoarse for every list, once"""
    prm = helpers.track_params(prob)
    return {k: cases.oracle_loop(oracle, prob, prm, cases.poses(xs), AFF0, [rm] * 5) for k, (xs, rm) in LISTS.items()}


@pytest.fixture()
def ctx(gpu_ctx, prob):
    gpu_ctx.upload_pyramid(cases.NEW_SLOT, prob["pyr_new"])
    gpu_ctx.set_ref(cases.REF_SLOT, prob["pc"])
    return gpu_ctx


def _run(ctx, prob, name, **kw):
    xs, rm = LISTS[name]
    tries = cases.poses(xs)
    rc, out, rmse, R = cases.new_coarse(ctx, helpers.track_params(prob), tries, AFF0, [rm] * 5, **kw)
    ctx.check(rc)
    return tries, out, rmse, R


def _pose_close(got, want, tol=1e-5):
    return np.abs(np.array(got) - np.array(want)).max() <= tol


def _same_bits(a, b):
    return all(ref.same_double(x, y) for x, y in zip(a, b))


def test_first_try_accepted_is_the_single_call(ctx, prob):
    """[G] with a large lastCoarseRMSE — the path of nearly every frame: bit-identical to sdso_track_newest_coarse with NaN bounds"""
    prm = helpers.track_params(prob)
    tries = cases.poses([cases.G])
    T = cases.se3_of(tries[0]); aff = abi.Aff(*AFF0); single = abi.TrackResult()
    ctx.check(ctx.L.sdso_track_newest_coarse(ctx.h, cases.REF_SLOT, cases.NEW_SLOT, C.byref(prm), C.byref(T), C.byref(aff), C.byref(single)))
    assert single.good == 1
    rc, out, rmse, R = cases.new_coarse(ctx, prm, tries, AFF0, [1e9] * 5)
    ctx.check(rc)
    assert (out.haveOneGood, out.winner, out.tryIterations) == (1, 0, 1)
    assert bytes(out.pose) == bytes(T) and bytes(out.aff) == bytes(aff)
    assert _same_bits(R[0].lastResiduals[:], single.lastResiduals[:]) and _same_bits(out.flowVecs[:], single.lastFlowIndicators[:])
    assert _same_bits(R[0].lastFlowIndicators[:], single.lastFlowIndicators[:])
    assert _same_bits(rmse, single.lastResiduals[:]) and _same_bits(out.achievedRes[:], single.lastResiduals[:])
    assert (R[0].ran, R[0].good, R[0].abort_lvl, R[0].winner) == (1, 1, -1, 1)
    # the trace: levels 3..0 in order (a repeated level twice), the last event of each level is that level's residual
    lv = [R[0].trace.lvl[e] for e in range(R[0].trace.n)]
    assert lv == sorted(lv, reverse=True) and set(lv) == {0, 1, 2, 3} and len(lv) <= 5
    for e, l in enumerate(lv):
        if e + 1 == len(lv) or lv[e + 1] != l:
            assert ref.same_double(R[0].trace.res[e], single.lastResiduals[l])
    # without records: the same result
    rc, out2, rmse2, _ = cases.new_coarse(ctx, prm, tries, AFF0, [1e9] * 5, with_recs=False)
    ctx.check(rc)
    assert bytes(out2) == bytes(out) and _same_bits(rmse2, rmse)


def test_hopeless_tries_first(ctx, prob, oracle_loops):
    """[H, H, G], lastCoarseRMSE = 1e9: the oracle's winner, its pose, its achievedRes; for H only the verdict (near-singular system)"""
    want = oracle_loops["HHG"]
    assert (want["winner"], want["tryIterations"], want["haveOneGood"]) == (2, 3, 1)
    tries, out, rmse, R = _run(ctx, prob, "HHG")
    print("achievedRes", out.achievedRes[:], "oracle", want["achievedRes"])
    assert (out.winner, out.tryIterations, out.haveOneGood) == (2, 3, 1)
    assert [R[k].ran for k in range(3)] == [1, 1, 1]
    assert [R[k].good for k in range(3)] == [s["good"] for s in want["seen"]] == [0, 0, 1]
    assert _pose_close(cases.se3_tuple(out.pose), want["pose"])
    assert abs(out.aff.a - want["aff"][0]) <= 1e-5 and abs(out.aff.b - want["aff"][1]) <= 1e-3
    for l in range(5):
        a, b = out.achievedRes[l], want["achievedRes"][l]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-5 * b, l
    assert _same_bits(rmse, out.achievedRes[:])


def test_good_try_first_aborts_the_hopeless_ones(ctx, prob, oracle_loops):
    """[G, H, H], lastCoarseRMSE = 0 (never stops): both H abort on level 3 under G's bounds"""
    want = oracle_loops["GHH"]
    assert (want["winner"], want["tryIterations"]) == (0, 3) and [s["abort_lvl"] for s in want["seen"]] == [-1, 3, 3]
    tries, out, rmse, R = _run(ctx, prob, "GHH")
    assert (out.winner, out.tryIterations, out.haveOneGood) == (0, 3, 1)
    for k in (1, 2):
        print("H under G's bounds: level 3 at", R[k].lastResiduals[3], "against 1.5 *", out.achievedRes[3])
        assert (R[k].ran, R[k].good, R[k].abort_lvl, R[k].winner) == (1, 0, 3, 0)
        assert all(np.isnan(R[k].lastResiduals[l]) for l in (0, 1, 2)) and np.isfinite(R[k].lastResiduals[3])
        assert bytes(R[k].pose) == bytes(cases.se3_of(tries[k])) and (R[k].aff.a, R[k].aff.b) == AFF0
    assert _pose_close(cases.se3_tuple(out.pose), want["pose"])
    assert abs(out.aff.a - want["aff"][0]) <= 1e-5 and abs(out.aff.b - want["aff"][1]) <= 1e-3


def test_no_good_try(ctx, prob, oracle_loops):
    """[H, H]: the ending of FullSystem.cpp:503-511"""
    want = oracle_loops["HH"]
    assert want["haveOneGood"] == 0
    xs, _ = LISTS["HH"]
    tries = cases.poses(xs)
    aff0 = (0.03, -1.5)
    rc, out, rmse, R = cases.new_coarse(ctx, helpers.track_params(prob), tries, aff0, [1e9] * 5)
    ctx.check(rc)
    assert (out.haveOneGood, out.winner, out.tryIterations) == (0, -1, 2)
    assert bytes(out.pose) == bytes(cases.se3_of(tries[0])) and (out.aff.a, out.aff.b) == aff0
    assert out.flowVecs[:] == [0.0, 0.0, 0.0]
    assert all(np.isnan(x) for x in out.achievedRes[:]) and all(np.isnan(x) for x in rmse)


def test_ties_follow_the_rules_on_the_calls_own_numbers(ctx, prob, oracle_loops):
    """[0, 2 truth, truth / 2, truth], lastCoarseRMSE = 0: every try converges to the same minimum and the winner is decided by
    differences of 1e-6 relative.  (a) the outputs are the rules applied to the returned per-try records, bit for bit; (b) twice the
    same bytes; (c) the winner is a try that ties with the oracle's winner in the oracle's own numbers, with that try's oracle pose."""
    want = oracle_loops["ties"]
    tries, out, rmse, R = _run(ctx, prob, "ties")
    n = len(tries)
    print("level-0 residuals", [R[k].lastResiduals[0] for k in range(n)], "oracle", [s["lastResiduals"][0] for s in want["seen"]], "winner", out.winner,
          "oracle", want["winner"])
    # (a) against sdso_track_tries_replay and against the Python loop on the same records
    R2 = (abi.TrackTry * n)()
    for k in range(n):
        R2[k].trace = R[k].trace; R2[k].end_good = R[k].end_good; R2[k].end_pose = R[k].end_pose; R2[k].end_aff = R[k].end_aff
    T = (abi.SE3 * n)(*[cases.se3_of(t) for t in tries])
    rc, out2, rmse2 = cases.replay(ctx.L, R2, T, AFF0, [0.0] * 5, 1.5)
    assert rc == 0
    assert bytes(out2) == bytes(out) and _same_bits(rmse2, rmse) and bytes(R2) == bytes(R)
    cases.assert_equal_to_ref(out, rmse, R, ref.track_new_coarse(cases.from_c(R), tries, AFF0, [0.0] * 5, 1.5))
    assert out.tryIterations == n and all(R[k].ran == 1 for k in range(n))
    # (b)
    _, out3, rmse3, R3 = _run(ctx, prob, "ties")
    assert bytes(out3) == bytes(out) and _same_bits(rmse3, rmse) and bytes(R3) == bytes(R)
    # (c)
    w = out.winner
    assert w >= 0 and want["seen"][w] is not None
    r_w, r_o = want["seen"][w]["lastResiduals"][0], want["seen"][want["winner"]]["lastResiduals"][0]
    assert abs(r_w - r_o) <= 1e-5 * r_o
    assert _pose_close(cases.se3_tuple(out.pose), want["seen"][w]["pose"])


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
        rc, out, rmse, R = cases.new_coarse(ctx, p, tries, AFF0, [0.0] * 5)
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
        rc = L.sdso_track_new_coarse(h, ref_slot, new_slot, C.byref(p) if p is not None else None, ntries, T, a, m if rm else None, 1.5,
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
    assert L.sdso_track_new_coarse(None, 1, 2, C.byref(prm), n, T, C.byref(a), (C.c_double * 5)(), 1.5, C.byref(abi.TrackTriesResult()), None) != 0
    after = good_call()
    assert before[0] == after[0] and before[1] == after[1] and _same_bits(before[2], after[2])
    p2 = helpers.track_params(prob)
    for i in range(5):
        p2.minResForAbort[i] = 0.01
    ignored = good_call(p2)
    assert before[0] == ignored[0] and before[1] == ignored[1] and _same_bits(before[2], ignored[2])
