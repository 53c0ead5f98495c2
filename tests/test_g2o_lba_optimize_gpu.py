"""sdso_g2o_lba_optimize — FullSystem::optimize as the fork compiles it (FullSystemOptimize.cpp:402-868) on the device — against
tests/g2o_lba_ref.py, the same algorithm in NumPy f64 over the CPU oracle's edge.

Integer outcomes (iterations, trials per iteration, stop reason, the active set, states, levels) must be EQUAL: the reference's margins
(tests/test_g2o_lba_ref.py) make them comparable.  Doubles (estimates, chi2 and lambda per iteration) may deviate by the order of the f64
sums and by the solve only.  BAR is 10 x the largest relative deviation measured over the cases A-F on an MI355X
(profiles/g2o_lba_optimize.txt) and may never exceed 1e-7: beyond that a flipped float rounding of a pair table or a wrong branch is
showing.  A deviation is relative to the largest magnitude of the reference array it belongs to (rotation, translation, affine pairs,
camera, idepth; chi2 and lambda entry by entry).
"""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import g2o_lba_ref as ref

pytestmark = pytest.mark.gpu

BAR = 2.9e-11       # 10 x 2.87e-12, the largest deviation over A-F (case C, translation); the cap is 1e-7
assert BAR <= 1e-7
NAMES = "ABCDEFG"
ERR_ARG = -1


def _slots(name):
    return [600 + 10 * NAMES.index(name) + f for f in range(ref.case(name)["nf"])]


@pytest.fixture(scope="module")
def uploaded(gpu_ctx):
    for name in NAMES:
        c = ref.case(name)
        for f, s in enumerate(_slots(name)):
            gpu_ctx.upload_pyramid(s, c["win"]["pyrs"][f][:1])
    return True


def _run(gpu_ctx, name, **kw):
    c = ref.case(name)
    W, P, S, out, a = ref.make_call(c, _slots(name), **kw)
    rc = gpu_ctx.L.sdso_g2o_lba_optimize(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S), C.byref(out))
    return rc, W, P, S, out, a


def _rel(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300)) if x.size else 0.0


def deviations(c, r, S, out, a):
    """the relative deviations of a call's doubles from the reference run r"""
    nf, it = c["nf"], r["iterations"]
    est = ref.estimates(S, a, nf)
    d = dict(R=_rel(np.array([T[0] for T in est["Twh"]]), np.array([T[0] for T in r["Twh"]])),
             t=_rel(np.array([T[1] for T in est["Twh"]]), np.array([T[1] for T in r["Twh"]])),
             aff_a=_rel([x[0] for x in est["host_aff"]], [x[0] for x in r["host_aff"]]),
             aff_b=_rel([x[1] for x in est["host_aff"]], [x[1] for x in r["host_aff"]]),
             cam=_rel(est["cam"], r["cam"]), idepth=_rel(est["idepth"], r["idepth"]),
             chi2_final=_rel([out.chi2_final], [r["chi2_final"]]))
    d["chi2"] = max([_rel([out.chi2[i]], [r["chi2"][i]]) for i in range(it)] or [0.0])
    d["lambda"] = max([_rel([out.lambda_[i]], [r["lambdas"][i]]) for i in range(it)] or [0.0])
    return d, est


@pytest.mark.parametrize("name", list(NAMES))
def test_matches_reference(gpu_ctx, oracle, uploaded, name):
    c = ref.case(name)
    r = ref.reference(oracle, name)
    rc, W, P, S, out, a = _run(gpu_ctx, name)
    gpu_ctx.check(rc)
    print(name, "iterations", out.iterations, r["iterations"], "trials", out.trials[:out.iterations], r["trials"], "stop", out.stop, r["stop"],
          "n_active", out.n_active, r["n_active"])
    d, est = deviations(c, r, S, out, a)
    print(name, "deviations", {k: "%.3g" % v for k, v in d.items()}, "rmse", out.rmse, r["rmse"])
    assert out.iterations == r["iterations"] and list(out.trials[:out.iterations]) == r["trials"] and out.stop == r["stop"]
    assert out.n_active == r["n_active"]
    assert np.array_equal(a["active"], r["active"].astype(np.uint8))
    assert np.array_equal(a["state"], r["state"]) and np.array_equal(a["level"], r["level"])
    for k, v in d.items():
        assert v <= BAR, (k, v)
    assert abs(float(out.rmse) - float(r["rmse"])) <= 2e-7 * float(r["rmse"])      # a float: one rounding of a double that is within BAR
    # float results: equal where the float pair tables of the final estimates are equal, within the bar elsewhere
    tabs = ref.pair_tables(c, est["Twh"], est["host_aff"])
    pair = c["host"] * c["nf"] + c["target"]
    same = np.ones(c["nr"], bool)
    for tg, tr in zip(tabs, r["tables"]):
        same &= np.all(tg[pair] == tr[pair], axis=1)
    print(name, "residuals on equal tables", int(same.sum()), "of", c["nr"])
    for key, rk in (("ih", "ih"), ("cpt", "cpt"), ("energy", "energy")):
        g, w = a[key], r[rk]
        assert np.array_equal(g[same], w[same]), key
        if not same.all():
            assert np.all(np.abs(g[~same].astype(np.float64) - w[~same]) <= BAR * np.maximum(np.abs(w[~same]), 1e-30)), key
    # a host without an active edge keeps its inputs, an inactive edge its idepth
    for h in range(c["nf"]):
        if h not in r["hosts"]:
            assert np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and np.array_equal(est["Twh"][h][1], c["Twh"][h][1])
            assert est["host_aff"][h] == c["host_aff"][h]
    assert np.array_equal(est["idepth"][~r["active"]], c["idepth"][~r["active"]])
    if name == "G":
        assert len(r["hosts"]) < c["nf"]


def test_two_calls_are_bit_identical(gpu_ctx, uploaded):
    runs = []
    for _ in range(2):
        rc, W, P, S, out, a = _run(gpu_ctx, "F")
        gpu_ctx.check(rc)
        runs.append((bytes(out)[:C.sizeof(abi.G2oLbaResult) - 6 * C.sizeof(C.c_void_p)], bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam),
                     a["idepth"].tobytes(), a["state"].tobytes(), a["energy"].tobytes(), a["cpt"].tobytes(), a["level"].tobytes(),
                     a["ih"].tobytes(), a["active"].tobytes()))
    assert runs[0] == runs[1]


def test_zero_iterations(gpu_ctx, oracle, uploaded):
    c = ref.case("F")
    rc, W, P, S, out, a = _run(gpu_ctx, "F", max_iterations=0)
    gpu_ctx.check(rc)
    r = ref.optimize(oracle, c, max_iterations=0)
    assert out.iterations == 0 and out.stop == ref.STOP_ITERATIONS and out.n_active == r["n_active"]
    est = ref.estimates(S, a, c["nf"])
    for h in range(c["nf"]):
        assert np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and np.array_equal(est["Twh"][h][1], c["Twh"][h][1]) and est["host_aff"][h] == c["host_aff"][h]
    assert np.array_equal(est["cam"], c["cam"]) and np.array_equal(est["idepth"], c["idepth"])
    # the evaluation at the inputs, through the same tables: equal bit for bit
    assert np.array_equal(a["state"], r["state"]) and np.array_equal(a["level"], r["level"]) and np.array_equal(a["active"], r["active"].astype(np.uint8))
    assert np.array_equal(a["energy"], r["energy"]) and np.array_equal(a["cpt"], r["cpt"]) and np.all(a["ih"] == 0)
    assert abs(out.chi2_final - r["chi2_final"]) <= BAR * r["chi2_final"]
    assert abs(float(out.rmse) - float(r["rmse"])) <= 2e-7 * float(r["rmse"])


def test_no_residuals(gpu_ctx, uploaded):
    c = dict(ref.case("C"))
    c["nr"] = 0
    for k in ("host", "target", "u", "v", "idepth"):
        c[k] = c[k][:0]
    c["color"] = c["color"][:0]; c["weights"] = c["weights"][:0]
    W, P, S, out, a = ref.make_call(c, _slots("C"))
    out.iterations, out.n_active, out.rmse = 9, 9, 9.0
    gpu_ctx.check(gpu_ctx.L.sdso_g2o_lba_optimize(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S), C.byref(out)))
    assert out.iterations == 0 and out.n_active == 0 and out.rmse == 0 and out.stop == ref.STOP_ITERATIONS
    est = ref.estimates(S, a, c["nf"])
    assert np.array_equal(est["cam"], c["cam"]) and all(np.array_equal(est["Twh"][h][1], c["Twh"][h][1]) for h in range(c["nf"]))


def test_no_active_edge(gpu_ctx, uploaded):
    c = dict(ref.case("C"))
    c["u"] = np.full_like(c["u"], -2000.0)
    W, P, S, out, a = ref.make_call(c, _slots("C"))
    gpu_ctx.check(gpu_ctx.L.sdso_g2o_lba_optimize(gpu_ctx.h, C.byref(W), C.byref(P), C.byref(S), C.byref(out)))
    assert out.iterations == 0 and out.n_active == 0 and out.chi2_final == 0 and out.rmse == 0
    assert np.all(a["active"] == 0) and np.all(a["level"] == 1) and np.all(a["state"] == 1) and np.all(a["ih"] == 0)
    est = ref.estimates(S, a, c["nf"])
    assert np.array_equal(est["cam"], c["cam"]) and np.array_equal(est["idepth"], c["idepth"])
    assert all(np.array_equal(est["Twh"][h][0], c["Twh"][h][0]) and est["host_aff"][h] == c["host_aff"][h] for h in range(c["nf"]))


def test_refusals(gpu_ctx, uploaded):
    c = ref.case("C")
    L, h = gpu_ctx.L, gpu_ctx.h

    def refused(edit, null=None):
        W, P, S, out, a = ref.make_call(c, _slots("C"))
        out.iterations = 55
        before = (bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam), a["idepth"].tobytes(), a["state"].tobytes())
        edit(W, P, S, out, a)
        args = [C.byref(W), C.byref(P), C.byref(S), C.byref(out)]
        if null is not None:
            args[null] = None
        assert L.sdso_g2o_lba_optimize(h, *args) == ERR_ARG
        assert L.sdso_last_error(h)
        assert out.iterations == 55 and a["state"].tobytes() == before[4]
        if not getattr(edit, "touches_estimates", False):
            assert (bytes(a["Twh"]), bytes(a["host_aff"]), bytes(S.cam), a["idepth"].tobytes()) == before[:4]

    def est(f):
        f.touches_estimates = True
        return f

    for k in range(4):
        refused(lambda *x: None, null=k)
    for fld in ("frame_slot", "Ttw", "target_aff", "ab_exposure", "host_b0", "frameEnergyTH", "host", "target", "u", "v", "color", "weights"):
        refused(lambda W, P, S, out, a, fld=fld: setattr(W, fld, None))
    for fld in ("Twh", "host_aff", "idepth"):
        refused(est(lambda W, P, S, out, a, fld=fld: setattr(S, fld, None)))
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


def test_lba_eval_at_the_returned_estimates_reproduces_the_outputs(gpu_ctx, uploaded):
    """the per-residual results ARE the edge at the returned estimates: sdso_g2o_lba_eval there gives them bit for bit"""
    c = ref.case("F")
    rc, W, P, S, out, a = _run(gpu_ctx, "F")
    gpu_ctx.check(rc)
    est = ref.estimates(S, a, c["nf"])
    pR, pt, pab = ref.pair_tables(c, est["Twh"], est["host_aff"])
    E = abi.G2oLba()
    E.nf, E.nr, E.w, E.h = c["nf"], c["nr"], c["w"], c["h"]
    E.cam[:] = [float(x) for x in est["cam"]]
    E.frame_slot = W.frame_slot
    E.pair_R, E.pair_t, E.pair_ab = abi.fp(pR), abi.fp(pt), abi.fp(pab)
    E.host_b0, E.frameEnergyTH, E.host, E.target, E.u, E.v, E.color, E.weights = W.host_b0, W.frameEnergyTH, W.host, W.target, W.u, W.v, W.color, W.weights
    E.idepth = abi.dp(est["idepth"])
    nr = c["nr"]
    err = np.zeros((nr, 8)); J = np.zeros((nr, 8, 13)); st = np.zeros(nr, np.uint8); en = np.zeros((nr, 2), np.float32)
    cpt = np.zeros((nr, 3), np.float32); ih = np.zeros(nr, np.float32); lv = np.zeros(nr, np.uint8)
    gpu_ctx.check(gpu_ctx.L.sdso_g2o_lba_eval(gpu_ctx.h, C.byref(E), abi.dp(err), abi.dp(J), abi.bp(st), abi.fp(en), abi.fp(cpt), abi.fp(ih), abi.bp(lv)))
    assert np.array_equal(st, a["state"]) and np.array_equal(en, a["energy"]) and np.array_equal(cpt, a["cpt"])
    assert np.all(lv <= a["level"])                      # the returned level is sticky over the call
    e2 = (err ** 2).sum(1)
    rho0 = np.where(e2 <= 81.0, e2, 2 * np.sqrt(e2) * 9.0 - 81.0)
    chi = rho0[a["active"] != 0].sum()
    assert abs(chi - out.chi2_final) <= 1e-12 * chi     # the same 8-vectors, summed in another order
