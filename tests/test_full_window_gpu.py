"""Immature-point activation at the full window of eight keyframes, bit for bit against the CPU oracle and statements: every output is
a decision, an integer, or a float produced per point in a fixed operation order, so no tolerance appears anywhere.

What only these cases reach: residual slots 4 .. 6 of activate_point (lanes 32 .. 55), host = 7, groups 4 .. 7 of ImmTraceArgs /
ImmActArgs, eight named hosts in one sdso_imm_trace, and the second copy back of sdso_imm_activate (more than SDSO_IMM_ACT_FIRST_COPY
selected candidates).  tests/test_full_window_ref.py asserts on the CPU side alone that the cases do reach them.

The resident sequence runs once per module (fixture `seq`); the tests assert on what it recorded."""
import copy
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import activate_ref as AR
import distmap_cases as DC
import full_window_cases as FW
import immature_ref as R
import test_imm_activate_gpu as TA
import test_stereo as TS

pytestmark = pytest.mark.gpu
SLOT_BATCH = 1610               # frames 0 .. nf-1 of a batch case
SLOT = 1620                     # frames 0 .. 7 of the resident window
ID_TRACED, ID_DOCTORED, ID_COMPOSED = 1700, 1710, 1720
ERR_ARG = -1
W, H = FW.W, FW.H


# ------------------------------------------------------------------ sdso_activate_points_batch
@pytest.mark.parametrize("name", FW.BATCH_NAMES)
def test_activate_points_batch_bit_exact(gpu_ctx, oracle, name):
    case = FW.batch(name)
    d, nf = case["d"], case["d"]["nf"]
    slots = [SLOT_BATCH + f for f in range(nf)]
    try:
        for f in range(nf):
            gpu_ctx.upload_pyramid(slots[f], [case["imgs"][f]])
        so, io, ro = FW.run_oracle(oracle, case)
        A, keep = TS._activate_struct(d, frame_slots=slots, dI=case["imgs"], minObs=case["min_obs"])
        n = A.n
        sg, ig, rg = np.full(n, 77, np.int8), np.full(n, -7, np.float32), np.full((n, nf), 77, np.uint8)
        gpu_ctx.check(gpu_ctx.L.sdso_activate_points_batch(gpu_ctx.h, C.byref(A), abi.ptr(sg), abi.fp(ig), abi.bp(rg)))
    finally:
        for s in slots:
            gpu_ctx.L.sdso_release_pyramid(gpu_ctx.h, s)
    print(name, "n", n, "statuses -1/0/1", [int((so == s).sum()) for s in (-1, 0, 1)], "status / res_state / idepth differ at",
          int((so != sg).sum()), int((ro != rg).any(axis=1).sum()), int((~((io == ig) | (np.isnan(io) & np.isnan(ig)))).sum()))
    assert np.array_equal(so, sg)
    assert np.array_equal(ro, rg)
    assert np.array_equal(io, ig, equal_nan=True)


# ------------------------------------------------------------------ the resident sequence
def _geoms(ids, geom):
    return TA._imm_geoms([(i, g) for i, g in zip(ids, geom)])


def _trace_key(ctx, c, ids, ngeom=None, geoms=None):
    counts = np.full(abi.IMM_NCOUNTS, -1, np.int32)
    rc = ctx.L.sdso_imm_trace(ctx.h, SLOT + 7, -1, len(ids) if ngeom is None else ngeom, _geoms(ids, c["key_geom"]) if geoms is None else geoms, abi.fp(c["K4"]),
                              abi.fp(c["Ki"]), c["baseline"], abi.ip(counts))
    return rc, counts


def _activate(ctx, win, ids, min_obs, min_act_dist):
    return ctx.imm_activate(min_obs=min_obs, min_act_dist=float(min_act_dist), **TA._args(win, ids, slots=[SLOT + f for f in range(8)]))


def _call(ctx, oracle, c, ids, m, min_obs):
    """one sdso_imm_activate + fetch next to one activate_ref.activate on c["win"] and the flat map list m (both continue in place).  The
    statement has no group for the newest frame; the device's is reported in the counts and must come back as it was."""
    counts, got = _activate(ctx, c["win"], ids, min_obs, c["min_act_dist"])
    want = AR.activate(oracle, c["win"], m, min_obs, c["min_act_dist"])
    want["counts"][9 + 7] = len(c["newest"]["u"])
    return dict(counts=counts, got=got, want=want, groups=TA._get(ctx, ids), ref_groups=copy.deepcopy(c["win"]["groups"][:7] + [c["newest"]]),
                map=DC.dm_get(ctx, W, H), ref_map=np.array(m, np.float32).reshape(H >> 1, W >> 1))


@pytest.fixture(scope="module")
def seq(gpu_ctx, oracle):
    ctx, L = gpu_ctx, gpu_ctx.L
    rec = {}
    nat, doc = FW.resident(doctored=False), FW.resident()
    all_ids = set()

    def ids_of(base):
        out = list(range(base, base + 8))
        all_ids.update(out)
        return out

    try:
        for f in range(8):
            ctx.upload_pyramid(SLOT + f, [nat["win"]["imgs"][f]])

        # ---- 1. the eight groups as they stand before the key frame; 2. one trace that names all eight
        ids = ids_of(ID_TRACED)
        TA._put(ctx, ids, nat["before_key"])
        rec["put"] = (TA._get(ctx, ids), copy.deepcopy(nat["before_key"]))
        nine = (abi.ImmGeom * 9)()
        rec["nine_geoms"] = _trace_key(ctx, nat, ids, ngeom=9, geoms=nine)[0]
        rec["after_nine_geoms"] = TA._get(ctx, ids)
        rc, counts = _trace_key(ctx, nat, ids)
        ctx.check(rc)
        rec["trace"] = dict(counts=counts, want_counts=nat["key_counts"], groups=TA._get(ctx, ids), ref_groups=copy.deepcopy(nat["win"]["groups"][:7] + [nat["newest"]]))

        # ---- 3. the map; 4. the call on the traced set as it is, against the statement
        pg, u, v, idp = nat["seeds"]
        DC.dm_make(ctx, W, H, nat["win"]["KRKi"], nat["win"]["Kt"], pg, u, v, idp)
        rec["natural"] = _call(ctx, oracle, nat, ids, FW.ref_map(nat), 2)
        TA._release(ctx, ids)

        # ---- 4. the doctored set (every gate of STEP 2, every exit of optimizeImmaturePoint): the call, 5. a second call on its result
        ids = ids_of(ID_DOCTORED)
        TA._put(ctx, ids, doc["win"]["groups"][:7] + [doc["newest"]])
        DC.dm_make(ctx, W, H, doc["win"]["KRKi"], doc["win"]["Kt"], pg, u, v, idp)
        m = FW.ref_map(doc)
        rec["doctored"] = _call(ctx, oracle, doc, ids, m, 2)
        rec["again"] = _call(ctx, oracle, doc, ids, m, 1)

        # ---- refusals: nine frames; the set and the map stay as they were
        before = (TA._get(ctx, ids), DC.dm_get(ctx, W, H))
        win9 = dict(doc["win"], groups=[None] * 9, flagged=np.zeros(9, np.uint8), KRKi=np.zeros((8, 3, 3), np.float32), Kt=np.zeros((8, 3), np.float32),
                    pair_R=np.zeros((81, 9), np.float32), pair_t=np.zeros((81, 3), np.float32), pair_aff=np.zeros((81, 2), np.float32))
        rec["nine_frames"] = ctx.imm_activate_raw(min_obs=1, min_act_dist=0.7, **TA._args(win9, ids + [ID_DOCTORED + 8], slots=[SLOT + f for f in range(8)] + [SLOT]))[0]
        rec["nine_frames_state"] = (before, (TA._get(ctx, ids), DC.dm_get(ctx, W, H)))
        TA._release(ctx, ids)

        # ---- 6. the route of the older entry points from the same doctored state
        cc = FW.resident()
        ids = ids_of(ID_COMPOSED)
        TA._put(ctx, ids, cc["win"]["groups"][:7] + [cc["newest"]])
        DC.dm_make(ctx, W, H, cc["win"]["KRKi"], cc["win"]["Kt"], pg, u, v, idp)
        dec, records = TA._composed(ctx, cc["win"], ids, 2, cc["min_act_dist"], slot=SLOT)
        rec["composed"] = dict(decision=dec, records=records, groups=TA._get(ctx, ids), map=DC.dm_get(ctx, W, H))
    finally:
        TA._release(ctx, sorted(all_ids))
        for f in range(8):
            L.sdso_release_pyramid(ctx.h, SLOT + f)
    return rec


def test_eight_groups_are_put_and_traced_in_one_call(seq):
    TA._same_groups(*seq["put"])
    r = seq["trace"]
    print("counts", r["counts"].tolist(), "statement", r["want_counts"].tolist())
    assert np.array_equal(r["counts"], r["want_counts"])
    TA._same_groups(r["groups"], r["ref_groups"])
    assert all(len(g["u"]) > 0 for g in r["groups"])


@pytest.mark.parametrize("which", ["natural", "doctored"])
def test_call_equals_the_statement_past_the_first_copy(seq, which):
    r = seq[which]
    first_copy = FW.abi_define("SDSO_IMM_ACT_FIRST_COPY")
    TA._same_call(r)                                            # all 17 counts, every decision byte, every record, the groups afterwards
    assert len(r["counts"]) == abi.IMM_ACT_NCOUNTS == 17
    assert np.array_equal(r["map"], r["ref_map"])
    assert r["counts"][4] == len(r["got"]["frame"]) > first_copy
    late = slice(first_copy, None)                              # the records of the second copy, on their own
    for k in TA.REC_EXACT + TA.REC_FLOAT:
        assert np.array_equal(r["got"][k][late], r["want"]["records"][k][late], equal_nan=(k in TA.REC_FLOAT)), k
    assert r["got"]["res_state"].shape[1] == 8


def test_newest_group_is_counted_and_left_alone(seq):
    for which in ("natural", "doctored", "again"):
        r = seq[which]
        assert r["counts"][16] == len(r["ref_groups"][7]["u"]) > 0
        assert R.same(r["groups"][7], r["ref_groups"][7]) is None, R.same(r["groups"][7], r["ref_groups"][7])


def test_second_call_continues_from_the_result(seq):
    r = seq["again"]
    TA._same_call(r)
    assert np.array_equal(r["map"], r["ref_map"])
    assert r["counts"][0] == seq["doctored"]["counts"][9:16].sum()


def test_call_equals_the_older_entry_points_on_the_device(seq):
    new, old = seq["doctored"], seq["composed"]
    assert np.array_equal(new["got"]["decision"], old["decision"])
    TA._same_records(new["got"], old["records"])
    TA._same_groups(new["groups"][:7], old["groups"][:7])
    assert np.array_equal(new["map"], old["map"])


def test_nine_frames_and_nine_geometries_are_refused(seq):
    assert seq["nine_frames"] == ERR_ARG and seq["nine_geoms"] == ERR_ARG
    TA._same_groups(seq["after_nine_geoms"], seq["put"][1])
    (g0, m0), (g1, m1) = seq["nine_frames_state"]
    TA._same_groups(g0, g1)
    assert np.array_equal(m0, m1)
