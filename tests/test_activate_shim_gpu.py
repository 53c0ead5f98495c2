"""sdso_shim::ImmaturePoints::upload / activatePointsMT (host/sdso_shim.h) driven by host/test_activate_shim.cpp on stand-in types: the
records it returns and the set it leaves equal the C-ABI path from Python exactly, and the caller's loop over the records builds the
pointHessians the CPU statement of activatePointsMT (tests/activate_ref.py) predicts."""

import numpy as np
import pytest

import activate_cases as AC
import activate_ref as AR
import distmap_cases as DC
import distmap_ref as D
import immature_cases as Cs
import immature_ref as R
import shim_driver
import synth

f32 = np.float32
W, H = Cs.W, Cs.H
MIN_OBS = 1                      # what the reference passes (FullSystem.cpp:790)
IN, OOB = 0, 1                   # ResState


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_activate_shim")


def test_activate_shim_driver_compiles():
    """CPU: upload / activatePointsMT of the shim + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_activate_shim")


@pytest.mark.gpu
def test_shim_activation_equals_the_abi_path_and_the_statement(gpu_ctx, oracle, driver, tmp_path):
    ctx, L = gpu_ctx, gpu_ctx.L
    c = AC.window(oracle)
    win, case = c["win"], c["case"]
    nf = 4
    T = [h_["T"] for h_ in case["hosts"][:3]] + [case["frames"][2]["T"]]
    poses = []
    for t in T:
        ti = synth.se3_inv(t)
        poses.append(np.concatenate([t[0].ravel(), t[1], ti[0].ravel(), ti[1]]))
    pg, su, sv, sid = c["seeds"]
    arrays = dict(meta=np.array([W, H, nf, MIN_OBS], np.int32), calib=np.concatenate([win["K4"], [c["min_act_dist"], 3.0]]).astype(f32),
                  poses=np.concatenate(poses).astype(np.float64), flagged=win["flagged"], pair_R=win["pair_R"], pair_t=win["pair_t"], pair_aff=win["pair_aff"])
    for k in range(nf):
        arrays["frame%d" % k] = win["imgs"][k]
    for k in range(nf - 1):
        arrays["group%d_f" % k], arrays["group%d_st" % k] = shim_driver.pack_points(win["groups"][k])
        arrays["seeds%d" % k] = np.stack([su[pg == k], sv[pg == k], sid[pg == k]], axis=1).astype(f32)
    r = shim_driver.run("test_activate_shim", tmp_path, arrays, mode="run")
    out = r.out

    # the geometries the driver formed from the poses (CoarseDistanceMap::geomOf) are the ones both comparisons use: frame 1's differs from
    # the case's crafted sideways geometry, so the window below is the driver's, not the case's
    geoms = out("geoms", f32).reshape(nf - 1, 12)
    KRKi0, Kt0 = DC.window_geoms(np.array([synth.se3_pack(x) for x in T]), tuple(float(x) for x in win["K4"]))
    assert np.allclose(geoms[:, :9], KRKi0.reshape(-1, 9), rtol=1e-5, atol=1e-4) and np.allclose(geoms[:, 9:], Kt0, rtol=1e-5, atol=1e-4)
    win["KRKi"], win["Kt"] = geoms[:, :9].reshape(-1, 3, 3).copy(), geoms[:, 9:].copy()

    ri, rf, rs = out("rec_i", np.int32).reshape(-1, 4), out("rec_f", f32).reshape(-1, 23), out("rec_rs", np.uint8).reshape(-1, nf)
    drv = dict(frame=ri[:, 0], index=ri[:, 1], status=ri[:, 2].astype(np.int8), lastTraceStatus=ri[:, 3].astype(np.uint8), idepth=rf[:, 0], u=rf[:, 1], v=rf[:, 2],
               my_type=rf[:, 3], idepth_min=rf[:, 4], idepth_max=rf[:, 5], energyTH=rf[:, 6], color=rf[:, 7:15], weights=rf[:, 15:23], res_state=rs)
    slots, ids = [945 + k for k in range(nf)], [180 + k for k in range(nf)]
    try:
        # ---- the C-ABI path from Python on the same state
        for k in range(nf):
            ctx.upload_pyramid(slots[k], [win["imgs"][k]])
        for k in range(nf - 1):
            ctx.imm_put(ids[k], win["groups"][k], W, H)
        DC.dm_make(ctx, W, H, win["KRKi"], win["Kt"], pg, su, sv, sid)
        counts, got = ctx.imm_activate(ids, slots, win["flagged"], win["KRKi"], win["Kt"], win["pair_R"], win["pair_t"], win["pair_aff"], W, H, win["K4"], MIN_OBS,
                                       float(c["min_act_dist"]))
        assert len(drv["frame"]) == counts[4] > 100
        for k in ("frame", "index", "status", "lastTraceStatus", "res_state"):
            assert np.array_equal(drv[k], got[k]), k
        for k in ("idepth", "u", "v", "my_type", "idepth_min", "idepth_max", "energyTH", "color", "weights"):
            assert np.array_equal(drv[k], got[k], equal_nan=True), k
        for k in range(nf - 1):
            a, b = shim_driver.unpack_points(out("h%d_f" % k, f32), out("h%d_st" % k, np.uint8)), ctx.imm_get(ids[k])
            assert R.same(a, b) is None, (k, R.same(a, b))
        assert np.array_equal(out("map", f32).reshape(H >> 1, W >> 1), DC.dm_get(ctx, W, H))
        assert r.stdout.split() == ["activated", str(counts[4]), "points"] + [str(counts[9 + k]) for k in range(nf - 1)]
    finally:
        for hid in ids:
            L.sdso_imm_release_host(ctx.h, hid)
        for s in slots:
            L.sdso_release_pyramid(ctx.h, s)

    # ---- the caller's loop against the CPU statement: the pointHessians every host gains
    _, _, m = D.make_distance_map(W, H, win["KRKi"], win["Kt"], pg, su, sv, sid)
    want = AR.activate(oracle, win, m, MIN_OBS, c["min_act_dist"])["records"]
    total = 0
    for k in range(nf - 1):
        pf, pi = out("ph%d_f" % k, f32).reshape(-1, 3), out("ph%d_i" % k, np.int32).reshape(-1, 3)
        sel = (want["frame"] == k) & (want["status"] == 1)
        assert len(pf) == sel.sum()
        assert np.array_equal(pf[:, 0], want["u"][sel]) and np.array_equal(pf[:, 1], want["v"][sel]) and np.array_equal(pf[:, 2], want["idepth"][sel])
        rs_w = want["res_state"][sel]
        mask = sum((rs_w[:, f] == IN).astype(np.int32) << f for f in range(nf))
        assert np.array_equal(pi[:, 0], mask)                                                    # the targets of the new PointFrameResiduals
        assert np.array_equal(pi[:, 1], np.where(rs_w[:, nf - 1] == IN, IN, OOB))                # lastResiduals[0].second: the newest frame
        prev = np.where(rs_w[:, nf - 2] == IN, IN, OOB) if k != nf - 2 else np.full(len(rs_w), OOB)
        assert np.array_equal(pi[:, 2], prev)                                                    # lastResiduals[1].second: the one before it
        total += len(pf)
    assert total == (want["status"] == 1).sum() > 50
