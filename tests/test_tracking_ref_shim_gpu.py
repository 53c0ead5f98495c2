"""sdso_shim::CoarseTracker::setCoarseTrackingRef(WindowedBA&, frameHessians, fh_right) and WindowedBA::writeBackProjections
(host/sdso_shim.h) driven by host/test_tracking_ref_shim.cpp on stand-in types.  The program runs twice on the same window: once with
writeBackProjections = false and the overload that reads the device-resident window, once with the full write-back and the overload
that walks the pointer graph.  FrameHessian::pointHessians of one host is not in the window's point order (two members of a
three-points-on-one-pixel group are swapped), so the templates only agree if the shim hands the pointHessians order down."""

import numpy as np
import pytest

import helpers
import shim_driver
import synth
import tracking_ref_window_cases as TC

ITS = 3


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_tracking_ref_shim")


def test_tracking_ref_shim_driver_compiles():
    """CPU: the new overload, writeBackProjections and the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_tracking_ref_shim")


def _arrays(case, swap):
    arrays = dict(meta=np.array([case["nf"], case["np"], case["nr"], case["w"], case["h"], ITS, case["solverMode"], case["levels"], swap[0], swap[1]], np.int32),
                  calib=np.concatenate([case["calib_value_scaled"], case["calib_value_zero"], [case["baseline"]]]).astype(np.float64))
    for k, dt in (("evalPT", np.float64), ("state", np.float64), ("state_zero", np.float64), ("ab_exposure", np.float32), ("frameEnergyTH", np.float32),
                  ("frameID", np.int32), ("res_point", np.int32), ("res_target", np.int32), ("host", np.int32), ("u", np.float32), ("v", np.float32),
                  ("idepth", np.float32), ("idepth_zero", np.float32), ("color", np.float32), ("weights", np.float32), ("hasDepthPrior", np.uint8),
                  ("res_state", np.uint8)):
        arrays[k] = np.ascontiguousarray(case[k], dt)
    for f, pyr in enumerate(list(case["pyrs"]) + [case["pyr_right"]]):
        for l, img in enumerate(pyr):
            arrays["img%d_l%d" % (f, l)] = np.ascontiguousarray(img, np.float32)
    return arrays


def _read(r, mode, levels):
    lv = [dict(zip(TC.KEYS, r.out("%s_l%d" % (mode, l), np.float32).reshape(4, -1))) for l in range(levels)]
    return r.out(mode + "_pcn", np.int32), lv, r.out(mode + "_info", np.float64)


@pytest.mark.gpu
def test_window_overload_equals_the_graph_overload(gpu_ctx, driver, tmp_path):
    ctx = gpu_ctx
    case = TC.with_triples(TC.make_case(nf=4, pts_per_kf=200, seed=3101))
    # ---- the C-ABI route from Python on the same window: which points are splatted where (the swap must sit in a 3-point pixel group)
    up = TC.upload(ctx, case, 76, 780)
    try:
        TC.optimize(ctx, up["wid"], ITS)
        post = TC.post_state(ctx, case, up["wid"])
        fwd, _ = TC.host_route(ctx, case, up, 91, post=post)
        groups = [g for g in helpers.pixel_groups(fwd["u"], fwd["v"], case["w"]) if len(g) >= 3]
        swap = None
        for g in groups:                                       # a group whose reversal of the first two members changes the float sum
            p = fwd["point"][g]
            if len(set(case["host"][p])) != 1:
                continue
            prod = (fwd["new_idepth"][g] * fwd["weight"][g]).astype(np.float32)
            a = np.float32(np.float32(prod[0] + prod[1]) + prod[2]); b = np.float32(np.float32(prod[0] + prod[2]) + prod[1])
            if a != b:
                swap = (int(p[1]), int(p[2]))
                break
        assert swap is not None and len(groups) >= 20
        order = np.arange(case["np"], dtype=np.int32)
        order[swap[0]], order[swap[1]] = order[swap[1]], order[swap[0]]     # pointHessians order of the driver, as window indices
        want, _ = TC.host_route(ctx, case, up, 92, order=order, post=post)
        lv_want, lv_fwd = TC.get_ref(ctx, 92, case["levels"]), TC.get_ref(ctx, 91, case["levels"])
        assert not np.array_equal(TC.bits(lv_want[0]["idepth"]), TC.bits(lv_fwd[0]["idepth"]))    # the window's own order gives another template
    finally:
        ctx.L.sdso_ba_release_window(ctx.h, 76)
        for s in range(780, 785):
            ctx.L.sdso_release_pyramid(ctx.h, s)
    # ---- the driver, both overloads
    arrays, out = _arrays(case, swap), {}
    for mode in ("window", "graph"):
        out[mode] = _read(shim_driver.run("test_tracking_ref_shim", tmp_path, arrays, mode), mode, case["levels"])
    (pcn_w, lv_w, info_w), (pcn_g, lv_g, info_g) = out["window"], out["graph"]
    assert np.array_equal(pcn_w, pcn_g) and pcn_w[0] > 100
    for l in range(case["levels"]):
        for k in TC.KEYS:
            assert np.array_equal(TC.bits(lv_w[l][k]), TC.bits(lv_g[l][k])), (l, k)
            assert np.array_equal(TC.bits(lv_w[l][k]), TC.bits(lv_want[l][k])), (l, k)           # ... and the C-ABI route in that order
    # refFrameID, firstCoarseRMSE, lastRef_aff_g2l, the exposure parameters: as the graph overload sets them
    assert np.array_equal(info_w[:7], info_g[:7]) and info_w[0] == 100 + case["nf"] - 1 and info_w[1] == -1
    assert info_w[7] == len(want["point"]) and info_w[8] == 0
    # writeBackProjections = false left centerProjectedTo alone; the full write-back filled it; both runs dropped the same residuals
    assert info_w[9] == 0 and info_g[9] > 0.4 * case["nr"] and info_w[10] == info_g[10] > 0
