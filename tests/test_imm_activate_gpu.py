"""sdso_imm_put_host / sdso_imm_activate / sdso_imm_activate_fetch against the CPU statement (tests/activate_ref.py) and against the
composition of the older entry points on the device, bit for bit: every output is a decision, an integer, or a float produced per point
in a fixed operation order, so no tolerance is involved anywhere.

One sequence runs once per module on the device and on the statement (fixture `seq`); the tests assert on what it recorded."""
import copy
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import activate_cases as AC
import activate_ref as AR
import distmap_cases as DC
import distmap_ref as D
import immature_cases as Cs
import immature_ref as R

pytestmark = pytest.mark.gpu
SLOT = 940                      # frames 0..3 of the window
SLOT_L3, SLOT_R3, SLOT_SMALL = 950, 951, 952
ERR_ARG, ERR_STATE = -1, -4
W, H = Cs.W, Cs.H
REC_EXACT = ("frame", "index", "status", "res_state", "lastTraceStatus")
REC_FLOAT = ("idepth", "u", "v", "my_type", "idepth_min", "idepth_max", "energyTH", "color", "weights")


def _put(ctx, ids, groups):
    for hid, S in zip(ids, groups):
        if S is not None:
            ctx.imm_put(hid, S, W, H)


def _release(ctx, ids):
    for hid in ids:
        ctx.L.sdso_imm_release_host(ctx.h, hid)


def _make_map(ctx, c):
    pg, u, v, idp = c["seeds"]
    DC.dm_make(ctx, W, H, c["win"]["KRKi"], c["win"]["Kt"], pg, u, v, idp)


def _args(win, ids, slots=None, **over):
    nf = len(win["groups"])
    a = dict(host_id=ids, frame_slot=slots if slots is not None else [SLOT + f for f in range(nf)], host_flagged=win["flagged"], KRKi=win["KRKi"], Kt=win["Kt"],
             pair_R=win["pair_R"], pair_t=win["pair_t"], pair_aff=win["pair_aff"], w=W, h=H, K4=win["K4"])
    a.update(over)
    return a


def _activate(ctx, win, ids, min_obs, min_act_dist, **over):
    counts, rec = ctx.imm_activate(min_obs=min_obs, min_act_dist=float(min_act_dist), **_args(win, ids, **over))
    return counts, rec


def _get(ctx, ids):
    return [ctx.imm_get(i) if ctx_has(ctx, i) else None for i in ids]


def ctx_has(ctx, hid):
    return ctx.L.sdso_imm_get(ctx.h, hid, C.byref(abi.TracePoints()), None) == 0


def _counts(ctx, ids):
    out = []
    for i in ids:
        n = C.c_int(-1)
        ctx.check(ctx.L.sdso_imm_count(ctx.h, i, C.byref(n)))
        out.append(n.value)
    return out


def _sub_window(win, frames):
    """the window restricted to `frames` (the last one is the newest)"""
    nf0, nf = len(win["groups"]), len(frames)
    pick = [a * nf0 + b for a in frames for b in frames]
    return dict(groups=[win["groups"][f] for f in frames[:-1]] + [None], imgs=[win["imgs"][f] for f in frames], flagged=win["flagged"][frames].copy(),
                KRKi=win["KRKi"][frames[:-1]].copy(), Kt=win["Kt"][frames[:-1]].copy(), pair_R=win["pair_R"][pick].copy(), pair_t=win["pair_t"][pick].copy(),
                pair_aff=win["pair_aff"][pick].copy(), K4=win["K4"], w=W, h=H)


def _imm_geoms(named):
    G = (abi.ImmGeom * max(1, len(named)))()
    for i, (hid, g) in enumerate(named):
        G[i].host_id = hid
        for k in ("KRKi", "Kt", "aff", "KRi", "t"):
            getattr(G[i], k)[:] = [float(x) for x in g[k]]
    return G


def _trace3(ctx, case, named):
    """frame 3 as a non-key frame on the named hosts"""
    ctx.check(ctx.L.sdso_imm_trace(ctx.h, SLOT_L3, SLOT_R3, len(named), _imm_geoms(named), abi.fp(case["K4"]), abi.fp(case["Ki"]), case["baseline"], None))


def _composed(ctx, win, ids, min_obs, min_act_dist, slot=SLOT):
    """The path of the older entry points: sdso_imm_get of every host, sdso_activate_select, sdso_activate_points_batch, one sdso_imm_remove
    per host; the window's frames are in the slots slot .. slot + nf - 1.  -> (decision, records)"""
    nf = len(ids)
    got = [ctx.imm_get(i) for i in ids[:nf - 1]]
    cat = lambda k: np.ascontiguousarray(np.concatenate([S[k] for S in got]))
    frame = np.concatenate([np.full(len(S["u"]), g, np.int32) for g, S in enumerate(got)])
    index = np.concatenate([np.arange(len(S["u"]), dtype=np.int32) for S in got])
    cand = dict(pg=frame, u=cat("u"), v=cat("v"), idepth_min=cat("idepth_min"), idepth_max=cat("idepth_max"), quality=cat("quality"),
                interval=cat("lastTracePixelInterval"), status=cat("lastTraceStatus"), my_type=cat("my_type"))
    sel = DC.dm_select(ctx, dict(w=W, h=H, KRKi=win["KRKi"], Kt=win["Kt"], flagged=win["flagged"], cand=cand, min_act_dist=min_act_dist, min_trace_quality=3.0))
    dec = sel["decision"]
    opt = np.nonzero(dec == D.SELECT)[0]
    ns = len(opt)
    rec = dict(frame=frame[opt].copy(), index=index[opt].copy())
    for k in AR.COPIED:
        rec[k] = np.ascontiguousarray(cat(k)[opt])
    A = abi.Activate()
    keep = [np.ascontiguousarray(win[k], np.float32) for k in ("pair_R", "pair_t", "pair_aff")] + [rec[k] for k in ("u", "v", "idepth_min", "idepth_max", "color", "weights", "energyTH")]
    A.nf, A.w, A.h, A.n, A.minObs = nf, W, H, ns, min_obs
    A.K[:] = [float(x) for x in win["K4"]]
    A.pair_R, A.pair_t, A.pair_aff = abi.fp(keep[0]), abi.fp(keep[1]), abi.fp(keep[2])
    A.u, A.v, A.idepth_min, A.idepth_max, A.color, A.weights, A.energyTH = [abi.fp(a) for a in keep[3:]]
    hosts = np.ascontiguousarray(rec["frame"], np.int32)
    A.host = abi.ip(hosts)
    slots = np.arange(slot, slot + nf, dtype=np.int32)
    A.frame_slot = abi.ip(slots)
    status, idepth, res_state = np.zeros(ns, np.int8), np.zeros(ns, np.float32), np.zeros((ns, nf), np.uint8)
    ctx.check(ctx.L.sdso_activate_points_batch(ctx.h, C.byref(A), abi.ptr(status), abi.fp(idepth), abi.bp(res_state)))
    rec.update(status=status, idepth=idepth, res_state=res_state)
    flags = (dec == D.DELETE)
    flags[opt] = (status != 0) | (rec["lastTraceStatus"] == R.OOB)
    for g, S in enumerate(got):
        fl = np.ascontiguousarray(flags[frame == g], np.uint8)
        ctx.check(ctx.L.sdso_imm_remove(ctx.h, ids[g], len(fl), abi.bp(fl)))
    return dec, rec


def _keep_all(S):
    """a state none of whose entries STEP 2 deletes or selects: finite intervals, IPS_UNINITIALIZED (not activatable, the host not flagged)"""
    S = copy.deepcopy(S)
    S["idepth_max"][~np.isfinite(S["idepth_max"])] = np.float32(1)
    S["lastTraceStatus"][:] = R.UNINITIALIZED
    return S


def _patterns(n):
    last = np.zeros(n, bool); last[-1] = True
    run = np.zeros(n, bool); run[-12:-3] = True
    every = np.zeros(n, bool); every[5::37] = True
    return dict(last=last, run_at_the_back=run, every_37th=every, all=np.ones(n, bool), none=np.zeros(n, bool))


@pytest.fixture(scope="module")
def seq(gpu_ctx, oracle):
    ctx, L = gpu_ctx, gpu_ctx.L
    rec = {}
    c0 = AC.window(oracle)
    case = c0["case"]
    F3 = case["frames"][3]
    all_ids = set()

    def ids_of(base, n=4):
        out = list(range(base, base + n))
        all_ids.update(out)
        return out

    try:
        for f in range(4):
            ctx.upload_pyramid(SLOT + f, [c0["win"]["imgs"][f]])
        ctx.upload_pyramid(SLOT_L3, [F3["left"]]); ctx.upload_pyramid(SLOT_R3, [F3["right"]])
        ctx.upload_pyramid(SLOT_SMALL, [np.ascontiguousarray(c0["win"]["imgs"][0][:240, :320])])

        # ---- 1. put / get; a put group traced on the device
        ids = ids_of(100)
        _put(ctx, ids, c0["win"]["groups"])
        rec["put_get"] = ([ctx.imm_get(i) for i in ids[:3]], copy.deepcopy(c0["win"]["groups"][:3]))
        ctx.imm_put(ids[3], c0["empty"], W, H)
        rec["put_empty"] = (_counts(ctx, ids), ctx.imm_get(ids[3]))
        rec["put_occupied"] = L.sdso_imm_put_host(ctx.h, ids[0], W, H, C.byref(abi.TracePoints()), None)
        _release(ctx, ids)
        ref = AC.window(oracle, doctored=False)["win"]["groups"][:3]             # the traced state as it is
        _put(ctx, ids, ref)
        _trace3(ctx, case, [(ids[j], F3["geom"][j]) for j in range(3)])
        R.trace(oracle, [(ref[j], F3["geom"][j]) for j in range(3)], F3["left"], F3["right"], case["K4"], case["Ki"], case["baseline"])
        rec["put_trace"] = ([ctx.imm_get(i) for i in ids[:3]], ref)
        _release(ctx, ids)

        # ---- 2. the call against the statement, minObs 1 and 2; 3. against the composition of the older entry points (minObs 2)
        rec["call"] = {}
        for min_obs in (1, 2):
            c = AC.window(oracle)
            ids = ids_of(110 + 10 * min_obs)
            _put(ctx, ids, c["win"]["groups"])
            _make_map(ctx, c)
            _, m = AC.ref_map(c)
            counts, got = _activate(ctx, c["win"], ids, min_obs, c["min_act_dist"])
            want = AR.activate(oracle, c["win"], m, min_obs, c["min_act_dist"])
            rec["call"][min_obs] = dict(counts=counts, got=got, want=want, groups=_get(ctx, ids), ref_groups=copy.deepcopy(c["win"]["groups"]), n=_counts(ctx, ids),
                                        map=DC.dm_get(ctx, W, H), ref_map=np.array(m, np.float32).reshape(H >> 1, W >> 1))
            if min_obs == 2:
                # ---- 5e. a second call on the result, then a trace: the counts and blobs are consistent after the in-place removal
                counts2, got2 = _activate(ctx, c["win"], ids, 1, c["min_act_dist"])
                want2 = AR.activate(oracle, c["win"], m, 1, c["min_act_dist"])
                _trace3(ctx, case, [(ids[j], F3["geom"][j]) for j in range(3)])
                R.trace(oracle, [(c["win"]["groups"][j], F3["geom"][j]) for j in range(3)], F3["left"], F3["right"], case["K4"], case["Ki"], case["baseline"])
                rec["again"] = dict(counts=counts2, got=got2, want=want2, groups=_get(ctx, ids), ref_groups=copy.deepcopy(c["win"]["groups"]),
                                    map=DC.dm_get(ctx, W, H), ref_map=np.array(m, np.float32).reshape(H >> 1, W >> 1))
                cc = AC.window(oracle)
                ids_c = ids_of(140)
                _put(ctx, ids_c, cc["win"]["groups"])
                _make_map(ctx, cc)
                dec_c, rec_c = _composed(ctx, cc["win"], ids_c, 2, cc["min_act_dist"])
                rec["composed"] = dict(decision=dec_c, records=rec_c, groups=_get(ctx, ids_c), map=DC.dm_get(ctx, W, H))
                _release(ctx, ids_c)
            _release(ctx, ids)

        # ---- 4. removal patterns on one group of 1037 entries (nf = 2, nothing selected: only the NaN-doctored entries leave)
        base = _keep_all(c0["win"]["groups"][0])
        w2 = _sub_window(c0["win"], [0, 3])
        w2["flagged"][:] = 0
        rec["patterns"] = {}
        for name, fl in _patterns(len(base["u"])).items():
            S = copy.deepcopy(base)
            S["idepth_max"][fl] = np.nan
            ids = ids_of(150, 2)
            w2["groups"] = [S, None]
            _put(ctx, ids, w2["groups"])
            _make_map(ctx, c0)
            counts, got = _activate(ctx, w2, ids, 1, c0["min_act_dist"], slots=[SLOT, SLOT + 3])
            want = copy.deepcopy(S)
            R.remove(want, fl)
            rec["patterns"][name] = dict(counts=counts, got=got, group=ctx.imm_get(ids[0]), want=want, nflag=int(fl.sum()))
            _release(ctx, ids)

        # ---- 5. edges: nf = 2 with minObs 1; a frame without a group, an empty group and a newest frame with a group of its own
        c = AC.window(oracle)
        w2 = _sub_window(c["win"], [1, 3])
        ids = ids_of(160, 2)
        _put(ctx, ids, w2["groups"])
        _make_map(ctx, c)
        _, m = AC.ref_map(c)
        counts, got = _activate(ctx, w2, ids, 1, c["min_act_dist"], slots=[SLOT + 1, SLOT + 3])
        rec["nf2"] = dict(counts=counts, got=got, want=AR.activate(oracle, w2, m, 1, c["min_act_dist"]), groups=_get(ctx, ids), ref_groups=copy.deepcopy(w2["groups"]))
        _release(ctx, ids)

        c = AC.window(oracle)
        newest = copy.deepcopy(c["win"]["groups"][1])
        c["win"]["groups"] = [c["win"]["groups"][0], None, c["empty"], None]
        ids = ids_of(170)
        _put(ctx, ids, c["win"]["groups"][:3] + [newest])
        _make_map(ctx, c)
        _, m = AC.ref_map(c)
        counts, got = _activate(ctx, c["win"], ids, 2, c["min_act_dist"])
        want = AR.activate(oracle, c["win"], m, 2, c["min_act_dist"])
        rec["gaps"] = dict(counts=counts, got=got, want=want, groups=_get(ctx, ids), ref_groups=copy.deepcopy(c["win"]["groups"]), newest=newest,
                           n_newest=len(newest["u"]))

        # ---- 6. refusals leave the set and the map as they were
        win = c["win"]
        before = (_get(ctx, ids), DC.dm_get(ctx, W, H))
        ctx.imm_put(179, c["empty"], 320, 240); all_ids.add(179)
        call = lambda **over: ctx.imm_activate_raw(min_obs=1, min_act_dist=0.7, **_args(win, ids, **over))[0]
        two = _sub_window(win, [0, 3])
        rec["refusals"] = dict(
            nf_1=ctx.imm_activate_raw(min_obs=1, min_act_dist=0.7, **_args(_sub_window(win, [3]), ids[3:], slots=[SLOT + 3]))[0],
            nf_9=ctx.imm_activate_raw(min_obs=1, min_act_dist=0.7, **_args(dict(win, groups=[None] * 9, flagged=np.zeros(9, np.uint8), KRKi=np.zeros((8, 3, 3), np.float32),
                                                                                 Kt=np.zeros((8, 3), np.float32), pair_R=np.zeros((81, 9), np.float32),
                                                                                 pair_t=np.zeros((81, 3), np.float32), pair_aff=np.zeros((81, 2), np.float32)),
                                                                            list(range(300, 309)), slots=[SLOT] * 9))[0],
            twice=call(host_id=[ids[0], ids[1], ids[0], ids[3]]),
            unknown_slot=call(frame_slot=[SLOT, SLOT + 1, 999, SLOT + 3]),
            small_pyramid=call(frame_slot=[SLOT, SLOT_SMALL, SLOT + 2, SLOT + 3]),
            small_group=call(host_id=[ids[0], 179, ids[2], ids[3]]),
            other_map=ctx.imm_activate_raw(min_obs=1, min_act_dist=0.7, **_args(two, [ids[0], ids[3]], slots=[SLOT_SMALL, SLOT_SMALL], w=320, h=240))[0])
        rec["refusals_state"] = (before, (_get(ctx, ids), DC.dm_get(ctx, W, H)))
        fresh = abi.Context(0)
        try:
            rec["fetch_before"] = fresh.L.sdso_imm_activate_fetch(fresh.h, C.byref(abi.ImmActivated()), None)
            fresh.upload_pyramid(SLOT, [win["imgs"][0]]); fresh.upload_pyramid(SLOT + 3, [win["imgs"][3]])
            rec["no_map"] = fresh.imm_activate_raw(min_obs=1, min_act_dist=0.7, **_args(two, [1, 2], slots=[SLOT, SLOT + 3]))[0]
        finally:
            fresh.close()
    finally:
        _release(ctx, sorted(all_ids))
        for s in [SLOT + f for f in range(4)] + [SLOT_L3, SLOT_R3, SLOT_SMALL]:
            L.sdso_release_pyramid(ctx.h, s)
    return rec


def _same_groups(got, want):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), j
        if a is not None:
            assert R.same(a, b) is None, "frame %d: %s differs" % (j, R.same(a, b))


def _same_records(got, want):
    for k in REC_EXACT:
        assert np.array_equal(got[k], want[k]), k
    for k in REC_FLOAT:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k], equal_nan=True), k


def _same_call(r):
    print("counts", r["counts"], "statement", r["want"]["counts"])
    assert np.array_equal(r["got"]["decision"], r["want"]["decision"])
    assert np.array_equal(r["counts"], r["want"]["counts"])
    _same_records(r["got"], r["want"]["records"])
    _same_groups(r["groups"], r["ref_groups"])


def test_put_then_get_returns_every_member(seq):
    got, want = seq["put_get"]
    _same_groups(got, want)
    assert sum(int(np.isnan(S["idepth_max"]).sum() + np.isnan(S["energyTH"]).sum()) for S in want) > 20      # NaNs travelled
    n, empty = seq["put_empty"]
    assert n == [1037, 259, 1, 0] and len(empty["u"]) == 0
    assert seq["put_occupied"] == ERR_ARG


def test_a_put_group_traces_like_the_statement(seq):
    _same_groups(*seq["put_trace"])


@pytest.mark.parametrize("min_obs", [1, 2])
def test_call_equals_the_statement(seq, min_obs):
    r = seq["call"][min_obs]
    _same_call(r)
    assert r["n"] == list(r["want"]["counts"][9:13])
    assert np.array_equal(r["map"], r["ref_map"])
    assert r["counts"][4] == len(r["got"]["frame"]) > 100 and r["counts"][4] % 4 != 0


def test_call_equals_the_older_entry_points_on_the_device(seq):
    new, old = seq["call"][2], seq["composed"]
    assert np.array_equal(new["got"]["decision"], old["decision"])
    _same_records(new["got"], old["records"])
    _same_groups(new["groups"][:3], old["groups"][:3])
    assert np.array_equal(new["map"], old["map"])


@pytest.mark.parametrize("name", ["last", "run_at_the_back", "every_37th", "all", "none"])
def test_removal_patterns(seq, name):
    r = seq["patterns"][name]
    n = len(r["want"]["u"])
    assert n == 1037 - r["nflag"]
    assert list(r["counts"][:5]) == [1037, n, r["nflag"], 0, 0] and r["counts"][8] == r["nflag"] and r["counts"][9] == n
    assert len(r["got"]["frame"]) == 0 and (r["got"]["decision"] == D.DELETE).sum() == r["nflag"]      # a fetch with empty arrays succeeds
    assert R.same(r["group"], r["want"]) is None, R.same(r["group"], r["want"])


def test_two_frames(seq):
    r = seq["nf2"]
    _same_call(r)
    assert r["got"]["res_state"].shape[1] == 2 and r["counts"][4] > 10


def test_missing_group_empty_group_and_a_newest_group(seq):
    r = seq["gaps"]
    # the statement has no group for the newest frame; the device's is reported in the counts and left as it was
    want = r["want"]["counts"].copy()
    want[9 + 3] = r["n_newest"]
    assert np.array_equal(r["counts"], want)
    assert np.array_equal(r["got"]["decision"], r["want"]["decision"])
    _same_records(r["got"], r["want"]["records"])
    _same_groups(r["groups"][:3], r["ref_groups"][:3])
    assert r["groups"][1] is None and len(r["groups"][2]["u"]) == 0
    assert R.same(r["groups"][3], r["newest"]) is None
    assert (r["got"]["frame"] == 0).all() and r["counts"][4] > 50


def test_second_call_and_trace_continue_from_the_result(seq):
    r = seq["again"]
    print("counts", r["counts"], "statement", r["want"]["counts"])
    assert np.array_equal(r["got"]["decision"], r["want"]["decision"])
    assert np.array_equal(r["counts"], r["want"]["counts"])
    _same_records(r["got"], r["want"]["records"])
    _same_groups(r["groups"], r["ref_groups"])                # after the trace
    assert np.array_equal(r["map"], r["ref_map"])


def test_refusals_leave_the_set_and_the_map_alone(seq):
    r = seq["refusals"]
    assert r == dict(nf_1=ERR_ARG, nf_9=ERR_ARG, twice=ERR_ARG, unknown_slot=ERR_ARG, small_pyramid=ERR_ARG, small_group=ERR_ARG, other_map=ERR_ARG), r
    assert seq["no_map"] == ERR_STATE and seq["fetch_before"] == ERR_STATE
    (g0, m0), (g1, m1) = seq["refusals_state"]
    _same_groups(g0, g1)
    assert np.array_equal(m0, m1)
