"""CoarseDistanceMap and the candidate selection of FullSystem::activatePointsMT on the device (csrc/distmap.hip) against
tests/distmap_ref.py.  Every output is an integer or a decision: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import distmap_cases as Cs
import distmap_ref as R
import synth
from sdso_amd import abi

f32 = np.float32


def _check_make(ctx, w, h, KRKi, Kt, pg, u, v, idepth):
    ref_map, ref_n, m = R.make_distance_map(w, h, KRKi, Kt, pg, u, v, idepth)
    n = Cs.dm_make(ctx, w, h, KRKi, Kt, pg, u, v, idepth)
    got = Cs.dm_get(ctx, w, h)
    assert n == ref_n
    assert np.array_equal(got, ref_map)
    return ref_map, ref_n, m


@pytest.mark.gpu
def test_make_distance_map_window_1232x368(gpu_ctx):
    """sdso_distmap_make + _get with the active points of an 8-keyframe synth window (~2 000 points), geometries from its poses."""
    win = synth.ba_window(w=1232, h=368, nf=8, pts_per_kf=250, seed=3001)
    KRKi, Kt = Cs.window_geoms(win["evalPT"], win["K"])
    act = win["host"] < win["nf"] - 1                                   # the newest frame's own points are skipped (:1230)
    ref_map, ref_n, _ = _check_make(gpu_ctx, 1232, 368, KRKi, Kt, win["host"][act], win["u"][act], win["v"][act], win["idepth"][act])
    assert 1000 < ref_n <= act.sum() and (ref_map == 0).sum() > 900 and (ref_map == 1000).sum() > 0 and ref_map.max() == 1000


@pytest.mark.gpu
def test_make_distance_map_640x480(gpu_ctx):
    case = Cs.selection_case(w=640, h=480, nhost=5, per_host=10, n_active=300, seed=5)
    a = case["active"]
    ref_map, ref_n, _ = _check_make(gpu_ctx, 640, 480, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    vals = set(np.unique(ref_map).astype(int))
    assert 200 < ref_n and {0, 1, 2, 3, 10, 20}.issubset(vals)


@pytest.mark.gpu
def test_make_distance_map_edge_cases(gpu_ctx):
    """No points at all; duplicates; seeds on the last row / column; points projecting outside; points behind the camera whose
    quotient is finite (every entry of the geometry negated: ptp[2] < 0, same quotient)."""
    w, h = 1232, 368
    w1, h1 = w >> 1, h >> 1
    G0 = np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]], f32)           # iu = int(0.5 u + 0.5)
    KRKi = np.array([G0, -G0], f32)
    Kt = np.array([[0.25, -0.25, 0], [-0.25, 0.25, 0]], f32)
    ref_map, ref_n, _ = _check_make(gpu_ctx, w, h, KRKi, Kt, np.zeros(0, np.int32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, f32))
    assert ref_n == 0 and (ref_map == 1000).all()
    u = np.array([400, 400, 400.4, 2 * (w1 - 1), 2 * (w1 - 1), 300, 2 * w1 + 50, -40, 100, 1, 900, 900, 0.2], f32)
    v = np.array([200, 200, 200.2, 200, 2 * (h1 - 1), 2 * (h1 - 1), 100, 50, 2 * h1 + 9, 1, 150, 150, 0.2], f32)
    pg = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0], np.int32)
    idp = np.array([0.1, 0.1, 0.3, 0, 0, 0, 0.1, 0.1, 0.1, 0.5, 0.2, 0.7, 0], f32)
    ref_map, ref_n, _ = _check_make(gpu_ctx, w, h, KRKi, Kt, pg, u, v, idp)
    assert ref_n == 8                                                   # duplicates count, the five outside (incl. iv = 0, iu = 0) do not
    assert ref_map[100, w1 - 1] == 0 and ref_map[100, w1 - 2] == 1000   # last column: a seed that does not propagate
    assert ref_map[h1 - 1, 150] == 0 and ref_map[h1 - 2, 150] == 1000   # last row
    assert ref_map[75, 450] == 0 and ref_map[75, 451] == 1              # behind the camera, finite quotient: a seed like any other


@pytest.mark.gpu
def test_add_into_dist_final_sequence(gpu_ctx):
    """sdso_distmap_add for a list of pixels = the reference's successive addIntoDistFinal calls (only newly set pixels propagate)."""
    case = Cs.selection_case(n_active=700, per_host=10, seed=21)
    a = case["active"]
    w, h = case["w"], case["h"]
    w1, h1 = w >> 1, h >> 1
    _, _, m = _check_make(gpu_ctx, w, h, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    rs = np.random.RandomState(4)
    iu = np.concatenate([rs.randint(1, w1 - 1, 300), [0, w1 - 1, 5, w1 - 2, 300, 300]]).astype(np.int32)
    iv = np.concatenate([rs.randint(1, h1 - 1, 300), [7, 9, 0, h1 - 1, 90, 90]]).astype(np.int32)
    before = np.array(m, f32).reshape(h1, w1)
    for x, y in zip(iu, iv):
        R.add_into(m, w1, h1, int(x), int(y))
    Cs.dm_add(gpu_ctx, iu, iv)
    got = Cs.dm_get(gpu_ctx, w, h)
    ref = np.array(m, f32).reshape(h1, w1)
    assert np.array_equal(got, ref)
    assert (ref < before).sum() > 20000                                 # the inserts did change the map
    # one at a time gives the same as the list
    Cs.dm_make(gpu_ctx, w, h, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    for x, y in zip(iu[:40], iv[:40]):
        Cs.dm_add(gpu_ctx, [x], [y])
    Cs.dm_add(gpu_ctx, iu[40:], iv[40:])
    assert np.array_equal(Cs.dm_get(gpu_ctx, w, h), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", sorted(Cs.REGIMES))
def test_activate_select(gpu_ctx, regime):
    """activatePointsMT STEP 2 at 1232x368, 7 hosts x 2 000 candidates: decision, n_selected, the re-grown map, and iu / iv of every
    candidate that reached the distance test."""
    case = Cs.selection_case(**Cs.REGIMES[regime])
    a = case["active"]
    w, h = case["w"], case["h"]
    ref_map, ref_n, m = _check_make(gpu_ctx, w, h, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    m0 = list(m)
    ref = Cs.ref_select(R, case, m)
    # ---- the reference's output is not vacuous
    n = len(ref["decision"])
    rows = np.bincount(ref["row"], minlength=6)
    print(regime, "seeds", ref_n, "rows", rows, "selected", ref["n_selected"], "of", n)
    assert (rows > 0).all(), rows                                        # every rule of the cascade decides somebody
    assert 0.03 * n <= ref["n_selected"] <= 0.9 * n
    flat = Cs.ref_select(R, case, list(m0), regrow=False)                # the same pass over the initial map, no re-growth
    assert not np.array_equal(flat["decision"] == R.SELECT, ref["decision"] == R.SELECT)
    assert {"dense_0.7": 1000 < ref_n < 1400, "mid_2": 1800 < ref_n < 2200, "sparse_4": 2900 < ref_n < 3500}[regime]
    # ---- the device
    got = Cs.dm_select(gpu_ctx, case)
    assert got["n_selected"] == ref["n_selected"]
    assert np.array_equal(got["decision"], ref["decision"])
    reached = ref["reached"]
    assert np.array_equal(got["iu"][reached], ref["iu"][reached]) and np.array_equal(got["iv"][reached], ref["iv"][reached])
    final = Cs.dm_get(gpu_ctx, w, h)
    assert np.array_equal(final, np.array(m, f32).reshape(h >> 1, w >> 1))
    assert (final < ref_map).any()


@pytest.mark.gpu
def test_activate_select_map_in_global_memory(gpu_ctx):
    """A level-1 map that does not fit the workgroup's LDS (1280x1024 -> 640x512 = 327 680 pixels) takes the kernel's other form."""
    case = Cs.selection_case(w=1280, h=1024, nhost=3, per_host=1200, n_active=1500, min_act_dist=2.0, seed=31)
    a = case["active"]
    w, h = case["w"], case["h"]
    _, _, m = _check_make(gpu_ctx, w, h, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    ref = Cs.ref_select(R, case, m)
    got = Cs.dm_select(gpu_ctx, case)
    assert ref["n_selected"] > 300 and got["n_selected"] == ref["n_selected"] and np.array_equal(got["decision"], ref["decision"])
    assert np.array_equal(Cs.dm_get(gpu_ctx, w, h), np.array(m, f32).reshape(h >> 1, w >> 1))


@pytest.mark.gpu
def test_state_is_per_context(gpu_ctx):
    """A second context making, selecting on and growing a different map leaves the first one's untouched."""
    c1 = Cs.selection_case(**Cs.REGIMES["mid_2"])
    c2 = Cs.selection_case(w=640, h=480, nhost=3, per_host=500, n_active=400, min_act_dist=1.0, seed=77)
    a1, a2 = c1["active"], c2["active"]
    ref1, _, m1 = _check_make(gpu_ctx, c1["w"], c1["h"], c1["KRKi"], c1["Kt"], a1["pg"], a1["u"], a1["v"], a1["idepth"])
    other = abi.Context(0)
    try:
        # no map yet on the new context: the existing error code, nothing launched
        buf = np.zeros((240, 320), f32)
        assert other.L.sdso_distmap_get(other.h, abi.fp(buf)) == -4
        one = np.array([5], np.int32)
        assert other.L.sdso_distmap_add(other.h, 1, abi.ip(one), abi.ip(one)) == -4
        ref2, _, m2 = _check_make(other, c2["w"], c2["h"], c2["KRKi"], c2["Kt"], a2["pg"], a2["u"], a2["v"], a2["idepth"])
        r2 = Cs.ref_select(R, c2, m2)
        g2 = Cs.dm_select(other, c2)
        assert np.array_equal(g2["decision"], r2["decision"]) and r2["n_selected"] > 50
        assert np.array_equal(Cs.dm_get(gpu_ctx, c1["w"], c1["h"]), ref1)          # the first context's map did not move
        r1 = Cs.ref_select(R, c1, m1)
        g1 = Cs.dm_select(gpu_ctx, c1)
        assert np.array_equal(g1["decision"], r1["decision"])
        assert np.array_equal(Cs.dm_get(other, c2["w"], c2["h"]), np.array(m2, f32).reshape(240, 320))
        assert np.array_equal(Cs.dm_get(gpu_ctx, c1["w"], c1["h"]), np.array(m1, f32).reshape(c1["h"] >> 1, c1["w"] >> 1))
    finally:
        other.close()


@pytest.mark.gpu
def test_bad_arguments_are_refused(gpu_ctx):
    case = Cs.selection_case(per_host=5, n_active=50, seed=3)
    a = case["active"]
    L = gpu_ctx.L
    G = abi.make_distmap_geoms(case["KRKi"], case["Kt"])
    pg = a["pg"].copy(); pg[3] = 7                                        # beyond ngeom
    ns = C.c_int(0)
    assert L.sdso_distmap_make(gpu_ctx.h, 1232, 368, 7, G, len(pg), abi.ip(pg), abi.fp(a["u"]), abi.fp(a["v"]), abi.fp(a["idepth"]), C.byref(ns)) == -1
    assert L.sdso_distmap_make(gpu_ctx.h, 1232, 368, 7, G, 5, None, abi.fp(a["u"]), abi.fp(a["v"]), abi.fp(a["idepth"]), C.byref(ns)) == -1
    Cs.dm_make(gpu_ctx, 1232, 368, case["KRKi"], case["Kt"], a["pg"], a["u"], a["v"], a["idepth"])
    before = Cs.dm_get(gpu_ctx, 1232, 368)
    bad = np.array([616], np.int32); ok = np.array([5], np.int32)
    assert L.sdso_distmap_add(gpu_ctx.h, 1, abi.ip(bad), abi.ip(ok)) == -1     # outside the level-1 map
    assert L.sdso_distmap_add(gpu_ctx.h, 1, abi.ip(ok), abi.ip(np.array([-1], np.int32))) == -1
    wrong = dict(case); wrong["w"] = 640; wrong["h"] = 480
    with pytest.raises(abi.SdsoError):
        Cs.dm_select(gpu_ctx, wrong)                                           # not the size the map was made for
    assert np.array_equal(Cs.dm_get(gpu_ctx, 1232, 368), before)
