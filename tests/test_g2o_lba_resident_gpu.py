"""sdso_g2o_lba_optimize_enqueue / _done / _fetch / _resident — the fork-live window optimiser with its Levenberg-Marquardt loop resident
on the device (csrc/g2o_lba_resident.hip) — against tests/g2o_lba_ref.py, against the host-driven sdso_g2o_lba_optimize on the same
inputs, and against its own enqueue contract.

Integer outcomes must be EQUAL (the reference's margins make them comparable); doubles may deviate by the order of the f64 sums, by the
solve and by the device's exp / sin / cos / pow only.  BAR_RES is 10 x the largest relative deviation of this call from the reference over
the cases A-F on an MI355X (profiles/g2o_lba_resident.txt has every case) and may never exceed 1e-7, the project's cap.  A deviation is
relative to the largest magnitude of the reference array it belongs to, as in test_g2o_lba_optimize_gpu.py, whose helpers are used.
"""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import g2o_lba_ref as ref
import test_g2o_lba_optimize_gpu as one

pytestmark = pytest.mark.gpu

BAR_RES = 2.9e-11       # 10 x 2.87e-12, the largest deviation over A-F (case C, translation); the cap is 1e-7
assert BAR_RES <= 1e-7
NAMES = "ABCDEFG"
ERR_ARG, ERR_STATE = -1, -4


_cases = {}
_windows = {}


def _case(name):
    """the case, built afresh for this module: ref.make_call hands a case's own arrays to the call wherever their type already fits, so a
    test that edits a call's arrays (the refusals, here and in test_g2o_lba_optimize_gpu.py, on case C) edits the shared case — and the
    shared WINDOW, because a case's `target` is its window's res_target itself: those refusals leave target[5] out of range in the window
    of C and E.  That window is therefore built once more for this module (1.4 s); the other windows, which no test edits, are shared."""
    if name not in _cases:
        shared = ref._windows
        if name in "CE":
            ref._windows = _windows
        try:
            _cases[name] = ref.build_case(name)
        finally:
            ref._windows = shared
    return _cases[name]


def _fresh(c):
    """a copy whose arrays a test may overwrite"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _reference(oracle, name):
    """the reference run of a case: ref.reference's, computed once and shared (from the case as built, if this module is the first to ask)"""
    if name not in ref._results:
        ref._results[name] = ref.optimize(oracle, _case(name))
    return ref._results[name]


def _slots(name):
    return [800 + 10 * NAMES.index(name) + f for f in range(_case(name)["nf"])]


@pytest.fixture(scope="module")
def uploaded(gpu_ctx):
    for name in NAMES:
        c = _case(name)
        for f, s in enumerate(_slots(name)):
            gpu_ctx.upload_pyramid(s, c["win"]["pyrs"][f][:1])
    return True


def _call(gpu_ctx, fn, c, slots, **kw):
    W, P, S, out, a = ref.make_call(c, slots, **kw)
    rc = getattr(gpu_ctx.L, fn)(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S), C.byref(out))
    return rc, W, P, S, out, a


def _resident(gpu_ctx, name, **kw):
    rc, W, P, S, out, a = _call(gpu_ctx, "sdso_g2o_lba_optimize_resident", _case(name), _slots(name), **kw)
    gpu_ctx.check(rc)
    return W, P, S, out, a


def _bytes(S, out, a):
    """every output of a call (the byte list of test_two_calls_are_bit_identical)"""
    return (bytes(out)[:C.sizeof(abi.G2oLbaResult) - 6 * C.sizeof(C.c_void_p)], bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam),
            a["idepth"].tobytes(), a["state"].tobytes(), a["energy"].tobytes(), a["cpt"].tobytes(), a["level"].tobytes(),
            a["ih"].tobytes(), a["active"].tobytes())


def _compare(c, r, S, out, a, bar, label):
    """integers equal, doubles within bar, floats equal on equal tables, the kept-input rules: test_matches_reference's body"""
    print(label, "iterations", out.iterations, r["iterations"], "trials", out.trials[:out.iterations], r["trials"], "stop", out.stop, r["stop"],
          "n_active", out.n_active, r["n_active"])
    d, est = one.deviations(c, r, S, out, a)
    print(label, "deviations", {k: "%.3g" % v for k, v in d.items()}, "largest %.3g" % max(d.values()), "rmse", out.rmse, r["rmse"])
    assert out.iterations == r["iterations"] and list(out.trials[:out.iterations]) == r["trials"] and out.stop == r["stop"]
    assert out.n_active == r["n_active"]
    assert np.array_equal(a["active"], r["active"].astype(np.uint8))
    assert np.array_equal(a["state"], r["state"]) and np.array_equal(a["level"], r["level"])
    for k, v in d.items():
        assert v <= bar, (k, v)
    assert abs(float(out.rmse) - float(r["rmse"])) <= 2e-7 * float(r["rmse"])      # a float: one rounding of a double that is within the bar
    tabs = ref.pair_tables(c, est["Twh"], est["host_aff"])
    pair = c["host"] * c["nf"] + c["target"]
    same = np.ones(c["nr"], bool)
    for tg, tr in zip(tabs, r["tables"]):
        same &= np.all(tg[pair] == tr[pair], axis=1)
    print(label, "residuals on equal tables", int(same.sum()), "of", c["nr"])
    for key in ("ih", "cpt", "energy"):
        g, w = a[key], r[key]
        assert np.array_equal(g[same], w[same]), key
        if not same.all():
            assert np.all(np.abs(g[~same].astype(np.float64) - w[~same]) <= bar * np.maximum(np.abs(w[~same]), 1e-30)), key
    for h in range(c["nf"]):                                                          # a host without an active edge keeps its inputs
        if h not in r["hosts"]:
            assert np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and np.array_equal(est["Twh"][h][1], c["Twh"][h][1])
            assert est["host_aff"][h] == c["host_aff"][h]
    assert np.array_equal(est["idepth"][~r["active"]], c["idepth"][~r["active"]])     # an inactive edge its idepth
    return d


# ------------------------------------------------------------------------------------------------ 1. the NumPy reference
@pytest.mark.parametrize("name", list(NAMES))
def test_matches_reference(gpu_ctx, oracle, uploaded, name):
    c = _case(name)
    r = _reference(oracle, name)
    W, P, S, out, a = _resident(gpu_ctx, name)
    _compare(c, r, S, out, a, BAR_RES, name)
    if name == "G":
        assert len(r["hosts"]) < c["nf"]


# ------------------------------------------------------------------------------------------------ 2. the host-driven call
@pytest.mark.parametrize("name", list(NAMES))
def test_matches_the_host_driven_call(gpu_ctx, uploaded, name):
    c = _case(name)
    W, P, S, out, a = _resident(gpu_ctx, name)
    rc, W1, P1, S1, out1, a1 = _call(gpu_ctx, "sdso_g2o_lba_optimize", c, _slots(name))
    gpu_ctx.check(rc)
    assert (out.iterations, out.stop, out.n_active) == (out1.iterations, out1.stop, out1.n_active)
    assert list(out.trials) == list(out1.trials)
    for k in ("active", "state", "level"):
        assert np.array_equal(a[k], a1[k]), k
    e, e1 = ref.estimates(S, a, c["nf"]), ref.estimates(S1, a1, c["nf"])
    h = dict(Twh=[(R, t) for R, t in e1["Twh"]], host_aff=e1["host_aff"], cam=e1["cam"], idepth=e1["idepth"], chi2_final=out1.chi2_final,
             chi2=list(out1.chi2), lambdas=list(out1.lambda_), iterations=out1.iterations)
    d, _ = one.deviations(c, h, S, out, a)
    print(name, "against the host-driven call", {k: "%.3g" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= BAR_RES + one.BAR, (k, v)


# ------------------------------------------------------------------------------------------------ 3. parameters the cases do not take
@pytest.mark.parametrize("name,kw", [("E", dict(max_trials=4)), ("C", dict(max_iterations=1))], ids=["E-4-trials", "C-1-iteration"])
def test_other_parameters(gpu_ctx, oracle, uploaded, name, kw):
    c = _case(name)
    r = ref.optimize(oracle, c, **kw)
    assert r["rhos"] and min(abs(x) for x in r["rhos"]) >= 1e-4 and all(abs(g - 1e-3) >= 1e-4 for g in r["gains"])     # the reference's margins
    if name == "E":
        assert r["stop"] == ref.STOP_TRIALS and r["trials"] == [4] and r["iterations"] == 1
    else:
        assert r["iterations"] == 1 and r["stop"] == ref.STOP_ITERATIONS
    W, P, S, out, a = _resident(gpu_ctx, name, **kw)
    _compare(c, r, S, out, a, BAR_RES, name + str(kw))


def test_zero_iterations(gpu_ctx, oracle, uploaded):
    c = _case("F")
    W, P, S, out, a = _resident(gpu_ctx, "F", max_iterations=0)
    r = ref.optimize(oracle, c, max_iterations=0)
    assert out.iterations == 0 and out.stop == ref.STOP_ITERATIONS and out.n_active == r["n_active"]
    est = ref.estimates(S, a, c["nf"])
    for h in range(c["nf"]):
        assert np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and np.array_equal(est["Twh"][h][1], c["Twh"][h][1]) and est["host_aff"][h] == c["host_aff"][h]
    assert np.array_equal(est["cam"], c["cam"]) and np.array_equal(est["idepth"], c["idepth"])
    # the evaluation at the inputs, through the same tables: equal bit for bit
    assert np.array_equal(a["state"], r["state"]) and np.array_equal(a["level"], r["level"]) and np.array_equal(a["active"], r["active"].astype(np.uint8))
    assert np.array_equal(a["energy"], r["energy"]) and np.array_equal(a["cpt"], r["cpt"]) and np.all(a["ih"] == 0)
    assert abs(out.chi2_final - r["chi2_final"]) <= BAR_RES * r["chi2_final"]
    assert abs(float(out.rmse) - float(r["rmse"])) <= 2e-7 * float(r["rmse"])


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_two_calls_are_bit_identical(gpu_ctx, uploaded):
    runs = []
    for _ in range(2):
        W, P, S, out, a = _resident(gpu_ctx, "F")
        runs.append(_bytes(S, out, a))
    assert runs[0] == runs[1]


def test_a_run_does_not_depend_on_the_run_before(gpu_ctx, uploaded):
    runs = []
    for name in "FCF":
        W, P, S, out, a = _resident(gpu_ctx, name)
        runs.append(_bytes(S, out, a))
    assert runs[0] == runs[2] and runs[0] != runs[1]


# ------------------------------------------------------------------------------------------------ 5. self-consistency
def _lba_eval(gpu_ctx, c, W, est):
    pR, pt, pab = ref.pair_tables(c, est["Twh"], est["host_aff"])
    E = abi.G2oLba()
    E.nf, E.nr, E.w, E.h = c["nf"], c["nr"], c["w"], c["h"]
    E.cam[:] = [float(x) for x in est["cam"]]
    E.frame_slot = W.frame_slot
    E.pair_R, E.pair_t, E.pair_ab = abi.fp(pR), abi.fp(pt), abi.fp(pab)
    E.host_b0, E.frameEnergyTH, E.host, E.target, E.u, E.v, E.color, E.weights = W.host_b0, W.frameEnergyTH, W.host, W.target, W.u, W.v, W.color, W.weights
    idp = np.ascontiguousarray(est["idepth"], np.float64)
    E.idepth = abi.dp(idp)
    nr = c["nr"]
    o = dict(err=np.zeros((nr, 8)), J=np.zeros((nr, 8, 13)), st=np.zeros(nr, np.uint8), en=np.zeros((nr, 2), np.float32), cpt=np.zeros((nr, 3), np.float32),
             ih=np.zeros(nr, np.float32), lv=np.zeros(nr, np.uint8))
    gpu_ctx.check(gpu_ctx.L.sdso_g2o_lba_eval(gpu_ctx.h, C.byref(E), abi.dp(o["err"]), abi.dp(o["J"]), abi.bp(o["st"]), abi.fp(o["en"]), abi.fp(o["cpt"]),
                                              abi.fp(o["ih"]), abi.bp(o["lv"])))
    return o


def test_lba_eval_at_the_returned_estimates_reproduces_the_outputs(gpu_ctx, uploaded):
    """the per-residual results ARE the edge at the returned estimates: sdso_g2o_lba_eval there gives them bit for bit"""
    c = _case("F")
    W, P, S, out, a = _resident(gpu_ctx, "F")
    o = _lba_eval(gpu_ctx, c, W, ref.estimates(S, a, c["nf"]))
    assert np.array_equal(o["st"], a["state"]) and np.array_equal(o["en"], a["energy"]) and np.array_equal(o["cpt"], a["cpt"])
    assert np.all(o["lv"] <= a["level"])                 # the returned level is sticky over the call
    e2 = (o["err"] ** 2).sum(1)
    rho0 = np.where(e2 <= 81.0, e2, 2 * np.sqrt(e2) * 9.0 - 81.0)
    chi = rho0[a["active"] != 0].sum()
    assert abs(chi - out.chi2_final) <= 1e-12 * chi      # the same 8-vectors, summed in another order


# ------------------------------------------------------------------------------------------------ 6. the enqueue contract
def _enqueue(gpu_ctx, W, P, S):
    return gpu_ctx.L.sdso_g2o_lba_optimize_enqueue(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S))


def _fetch(gpu_ctx, S, out):
    return gpu_ctx.L.sdso_g2o_lba_optimize_fetch(gpu_ctx.h, C.byref(S), C.byref(out))


def test_the_inputs_are_copied_at_enqueue(gpu_ctx, uploaded):
    c = _case("F")
    W0, P0, S0, out0, a0 = _resident(gpu_ctx, "F")
    W, P, S, out, a = ref.make_call(_fresh(c), _slots("F"))
    gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
    for k in ("ab_exposure", "host_b0", "frameEnergyTH", "u", "v", "color", "weights", "idepth"):
        a[k][...] = np.nan
    for k in ("frame_slot", "host", "target"):
        a[k][...] = -1
    for k in ("Ttw", "Twh", "target_aff", "host_aff"):
        C.memset(a[k], 0xff, C.sizeof(a[k]))                    # NaN in every double
    C.memset(C.byref(P), 0, C.sizeof(P))
    C.memset(C.byref(W), 0, C.sizeof(W))
    S.cam[:] = [float("nan")] * 4
    W2, P2, S2, out2, a2 = ref.make_call(c, _slots("F"))        # where the results go: arrays of the sizes the job was enqueued with
    gpu_ctx.check(_fetch(gpu_ctx, S2, out2))
    assert _bytes(S2, out2, a2) == _bytes(S0, out0, a0)


def test_other_calls_between_enqueue_and_fetch_leave_the_job_alone(gpu_ctx, uploaded):
    c = _case("F")
    W0, P0, S0, out0, a0 = _resident(gpu_ctx, "F")
    W, P, S, out, a = ref.make_call(c, _slots("F"))
    gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
    rc, Wc, Pc, Sc, outc, ac = _call(gpu_ctx, "sdso_g2o_lba_optimize", _case("C"), _slots("C"))     # takes the ctx's scratch
    gpu_ctx.check(rc)
    assert outc.iterations > 0
    _lba_eval(gpu_ctx, c, W0, ref.estimates(S0, a0, c["nf"]))
    gpu_ctx.upload_pyramid(899, _case("C")["win"]["pyrs"][0][:1])                                   # an unrelated slot
    gpu_ctx.check(_fetch(gpu_ctx, S, out))
    assert _bytes(S, out, a) == _bytes(S0, out0, a0)
    gpu_ctx.check(gpu_ctx.L.sdso_release_pyramid(gpu_ctx.h, 899))


def test_one_job_per_ctx(gpu_ctx, uploaded):
    c = _case("F")
    W0, P0, S0, out0, a0 = _resident(gpu_ctx, "F")
    W, P, S, out, a = ref.make_call(c, _slots("F"))
    gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
    Wc, Pc, Sc, outc, ac = ref.make_call(_case("C"), _slots("C"))
    outc.iterations = 55
    before = _bytes(Sc, outc, ac)
    assert _enqueue(gpu_ctx, Wc, Pc, Sc) == ERR_STATE and gpu_ctx.L.sdso_last_error(gpu_ctx.h)
    assert gpu_ctx.L.sdso_g2o_lba_optimize_resident(gpu_ctx.h, C.byref(Wc), C.byref(Pc), C.byref(Sc), C.byref(outc)) == ERR_STATE
    assert _bytes(Sc, outc, ac) == before
    gpu_ctx.check(_fetch(gpu_ctx, S, out))                      # the first job, intact
    assert _bytes(S, out, a) == _bytes(S0, out0, a0)


def test_no_job(gpu_ctx, uploaded):
    L, h = gpu_ctx.L, gpu_ctx.h
    c = _case("C")
    W, P, S, out, a = ref.make_call(c, _slots("C"))
    out.iterations = 55
    before = _bytes(S, out, a)
    assert _fetch(gpu_ctx, S, out) == ERR_STATE and L.sdso_last_error(h)
    assert L.sdso_g2o_lba_optimize_done(h) == ERR_STATE
    assert _bytes(S, out, a) == before
    gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
    gpu_ctx.check(L.sdso_ctx_sync(h))
    assert L.sdso_g2o_lba_optimize_done(h) == 1                 # (e) after a synchronisation of the stream the job has finished
    gpu_ctx.check(_fetch(gpu_ctx, S, out))
    assert out.iterations == 4
    W2, P2, S2, out2, a2 = ref.make_call(c, _slots("C"))
    out2.iterations = 55
    before = _bytes(S2, out2, a2)
    assert _fetch(gpu_ctx, S2, out2) == ERR_STATE               # a second fetch
    assert L.sdso_g2o_lba_optimize_done(h) == ERR_STATE
    assert _bytes(S2, out2, a2) == before


@pytest.mark.parametrize("split", [False, True], ids=["resident", "enqueue-fetch"])
def test_no_residuals(gpu_ctx, uploaded, split):
    c = dict(_case("C"))
    c["nr"] = 0
    for k in ("host", "target", "u", "v", "idepth"):
        c[k] = c[k][:0]
    c["color"] = c["color"][:0]; c["weights"] = c["weights"][:0]
    W, P, S, out, a = ref.make_call(c, _slots("C"))
    out.iterations, out.n_active, out.rmse = 9, 9, 9.0
    if split:
        gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
        assert gpu_ctx.L.sdso_g2o_lba_optimize_done(gpu_ctx.h) == 1
        gpu_ctx.check(_fetch(gpu_ctx, S, out))
    else:
        gpu_ctx.check(gpu_ctx.L.sdso_g2o_lba_optimize_resident(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S), C.byref(out)))
    assert out.iterations == 0 and out.n_active == 0 and out.rmse == 0 and out.stop == ref.STOP_ITERATIONS
    est = ref.estimates(S, a, c["nf"])
    assert np.array_equal(est["cam"], c["cam"]) and all(np.array_equal(est["Twh"][h][1], c["Twh"][h][1]) for h in range(c["nf"]))
    assert _fetch(gpu_ctx, S, out) == ERR_STATE


def test_no_active_edge(gpu_ctx, uploaded):
    c = dict(_case("C"))
    c["u"] = np.full_like(c["u"], -2000.0)
    rc, W, P, S, out, a = _call(gpu_ctx, "sdso_g2o_lba_optimize_resident", c, _slots("C"))
    gpu_ctx.check(rc)
    assert out.iterations == 0 and out.n_active == 0 and out.chi2_final == 0 and out.rmse == 0
    assert np.all(a["active"] == 0) and np.all(a["level"] == 1) and np.all(a["state"] == 1) and np.all(a["ih"] == 0)
    est = ref.estimates(S, a, c["nf"])
    assert np.array_equal(est["cam"], c["cam"]) and np.array_equal(est["idepth"], c["idepth"])
    assert all(np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and est["host_aff"][h] == c["host_aff"][h] for h in range(c["nf"]))


def test_destroy_with_a_job_pending(gpu_ctx, uploaded):
    c = _case("C")
    ctx = abi.Context(0)
    try:
        slots = [10 + f for f in range(c["nf"])]
        for f, s in enumerate(slots):
            ctx.upload_pyramid(s, c["win"]["pyrs"][f][:1])
        W, P, S, out, a = ref.make_call(c, slots)
        ctx.check(ctx.L.sdso_g2o_lba_optimize_enqueue(ctx.h, C.byref(W), C.byref(P), C.byref(S)))
    finally:
        ctx.close()                                             # never fetched: the stream is drained, the job freed
    W, P, S, out, a = _resident(gpu_ctx, "C")
    assert out.iterations == 4


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("fn", ["sdso_g2o_lba_optimize_enqueue", "sdso_g2o_lba_optimize_resident"])
def test_refusals(gpu_ctx, uploaded, fn):
    """the list of test_g2o_lba_optimize_gpu.py::test_refusals; _enqueue takes no `out`, so the entries that null one do not apply to it"""
    c = _case("C")
    L, h = gpu_ctx.L, gpu_ctx.h
    has_out = fn.endswith("resident")

    def refused(edit, null=None):
        W, P, S, out, a = ref.make_call(_fresh(c), _slots("C"))
        out.iterations = 55
        before = (bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam), a["idepth"].tobytes(), a["state"].tobytes())
        edit(W, P, S, out, a)
        args = [C.byref(W), C.byref(P), C.byref(S)] + ([C.byref(out)] if has_out else [])
        if null is not None:
            args[null] = None
        assert getattr(L, fn)(h, *args) == ERR_ARG
        assert L.sdso_last_error(h)
        assert out.iterations == 55 and a["state"].tobytes() == before[4]
        if not getattr(edit, "touches_estimates", False):
            assert (bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam), a["idepth"].tobytes()) == before[:4]
        assert L.sdso_g2o_lba_optimize_done(h) == ERR_STATE     # no job left
        W2, P2, S2, out2, a2 = ref.make_call(c, _slots("C"))
        assert _fetch(gpu_ctx, S2, out2) == ERR_STATE

    def est(f):
        f.touches_estimates = True
        return f

    for k in range(4 if has_out else 3):
        refused(lambda *x: None, null=k)
    for fld in ("frame_slot", "Ttw", "target_aff", "ab_exposure", "host_b0", "frameEnergyTH", "host", "target", "u", "v", "color", "weights"):
        refused(lambda W, P, S, out, a, fld=fld: setattr(W, fld, None))
    for fld in ("Twh", "host_aff", "idepth"):
        refused(est(lambda W, P, S, out, a, fld=fld: setattr(S, fld, None)))
    if has_out:
        for fld in ("state", "energy", "centerProjectedTo", "edge_level", "idepth_hessian", "active"):
            refused(lambda W, P, S, out, a, fld=fld: setattr(out, fld, None))
    refused(lambda W, P, S, out, a: setattr(W, "nf", 0))
    refused(lambda W, P, S, out, a: setattr(W, "nf", 9))
    refused(lambda W, P, S, out, a: setattr(W, "nr", -1))
    refused(lambda W, P, S, out, a: a["frame_slot"].__setitem__(1, 99999))       # unknown slot
    refused(lambda W, P, S, out, a: setattr(W, "w", 320))                         # size mismatch
    refused(lambda W, P, S, out, a: a["host"].__setitem__(3, c["nf"]))
    refused(lambda W, P, S, out, a: a["host"].__setitem__(3, -1))
    refused(lambda W, P, S, out, a: a["target"].__setitem__(5, c["nf"]))
    refused(lambda W, P, S, out, a: a["u"].__setitem__(2, np.nan))
    refused(lambda W, P, S, out, a: a["v"].__setitem__(2, np.inf))
    refused(est(lambda W, P, S, out, a: a["idepth"].__setitem__(7, np.nan)))
    refused(est(lambda W, P, S, out, a: S.cam.__setitem__(1, float("nan"))))
    refused(est(lambda W, P, S, out, a: a["Twh"][1].t.__setitem__(0, float("inf"))))
    refused(est(lambda W, P, S, out, a: setattr(a["host_aff"][0], "a", float("nan"))))
    refused(lambda W, P, S, out, a: a["Ttw"][0].R.__setitem__(4, float("nan")))
    refused(lambda W, P, S, out, a: setattr(a["target_aff"][1], "b", float("nan")))
    refused(lambda W, P, S, out, a: setattr(P, "max_iterations", -1))
    refused(lambda W, P, S, out, a: setattr(P, "max_trials", 0))
    # a fetch with a null argument or array is refused and the job stays
    W, P, S, out, a = ref.make_call(c, _slots("C"))
    gpu_ctx.check(_enqueue(gpu_ctx, W, P, S))
    assert L.sdso_g2o_lba_optimize_fetch(h, None, C.byref(out)) == ERR_ARG
    out.state = None
    assert _fetch(gpu_ctx, S, out) == ERR_ARG
    out.state = abi.bp(a["state"])
    gpu_ctx.check(_fetch(gpu_ctx, S, out))
    assert out.iterations == 4
