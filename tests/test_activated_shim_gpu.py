"""The device-to-device keyframe hand-over through host/sdso_shim.h, driven by host/test_activated_shim.cpp on stand-in types:
CoarseDistanceMap::makeDistanceMap(WindowedBA&, ...) -> ImmaturePoints::activatePointsMT -> WindowedBA::updateActivated.  The driver's
caller loop builds the new PointHessians from the integer members of the records alone (their floats stay zero on the host), and the window
it leaves equals, bit for bit, the one the all-host C-ABI route makes from Python: sdso_ba_get_state + sdso_distmap_make, sdso_imm_activate +
fetch, stage 7 in NumPy, sdso_ba_window_update."""
import numpy as np
import pytest

import activate_cases as AC
import distmap_cases as DC
import immature_cases as Cs
import shim_driver
import synth
import window_activated_helpers as wa
import window_update_helpers as wu

f32 = np.float32
W, H = Cs.W, Cs.H
WID = 19
SLOT = 2380
IDS = [2460, 2461, 2462, 2463]


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_activated_shim")


def test_activated_shim_driver_compiles():
    """CPU: the new shim members and their driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_activated_shim")


@pytest.mark.gpu
def test_shim_hand_over_equals_the_all_host_route(gpu_ctx, oracle, driver, tmp_path):
    ctx = gpu_ctx
    win = synth.ba_window(w=W, h=H, nf=4, pts_per_kf=40, seed=4101)
    c = AC.window(oracle)
    aw, case = c["win"], c["case"]
    nf = 4
    arrays = dict(meta=np.array([nf, win["np"], win["nr"], W, H, 0, win["solverMode"]], np.int32),
                  calib=np.concatenate([win["calib_value_scaled"], win["calib_value_zero"]]).astype(np.float64))
    for k in ("evalPT", "state", "state_zero"):
        arrays[k] = np.asarray(win[k], np.float64)
    for k in ("ab_exposure", "frameEnergyTH", "u", "v", "idepth", "idepth_zero", "color", "weights"):
        arrays[k] = np.asarray(win[k], f32)
    for k in ("frameID", "res_point", "res_target", "host"):
        arrays[k] = np.asarray(win[k], np.int32)
    for k in ("hasDepthPrior", "res_state"):
        arrays[k] = np.asarray(win[k], np.uint8)
    for f in range(nf):
        arrays["img%d_l0" % f] = np.asarray(win["pyrs"][f][0], f32)
    T = [h_["T"] for h_ in case["hosts"][:3]] + [case["frames"][2]["T"]]
    poses = []
    for t in T:
        ti = synth.se3_inv(t)
        poses.append(np.concatenate([t[0].ravel(), t[1], ti[0].ravel(), ti[1]]))
    arrays.update(a_meta=np.array([1], np.int32), a_calib=np.concatenate([aw["K4"], [c["min_act_dist"], 3.0]]).astype(f32),
                  a_poses=np.concatenate(poses).astype(np.float64), a_flagged=aw["flagged"], a_pair_R=aw["pair_R"], a_pair_t=aw["pair_t"], a_pair_aff=aw["pair_aff"])
    for k in range(nf):
        arrays["a_frame%d" % k] = aw["imgs"][k]
    for k in range(nf - 1):
        arrays["a_group%d_f" % k], arrays["a_group%d_st" % k] = shim_driver.pack_points(aw["groups"][k])
    r = shim_driver.run("test_activated_shim", tmp_path, arrays, mode="run")
    print(r.stdout.strip())
    out = r.out
    geoms = out("geoms", f32).reshape(nf - 1, 12)                 # CoarseDistanceMap::geomOf on the driver's poses: both routes use these
    KRKi, Kt = geoms[:, :9].reshape(-1, 3, 3).copy(), geoms[:, 9:].copy()
    aw["KRKi"], aw["Kt"] = KRKi, Kt

    slots = [SLOT + k for k in range(nf)]
    try:
        # ---- the all-host route from Python
        wu.upload_pyramids(ctx, win)
        wu.upload(ctx, win, WID)
        for k in range(nf):
            ctx.upload_pyramid(slots[k], [aw["imgs"][k]])
        for k in range(nf - 1):
            ctx.imm_put(IDS[k], aw["groups"][k], W, H)
        idp = np.zeros(win["np"], f32)
        ctx.check(ctx.L.sdso_ba_get_state(ctx.h, WID, None, wu.abi.fp(idp), None))
        seeds = win["host"] < nf - 1
        n_items = DC.dm_make(ctx, W, H, KRKi, Kt, win["host"][seeds], win["u"][seeds], win["v"][seeds], idp[seeds])
        assert out("num_items", np.int32)[0] == n_items > 0
        assert np.array_equal(out("map0", f32).reshape(H >> 1, W >> 1), DC.dm_get(ctx, W, H))
        counts, rec = ctx.imm_activate(IDS, slots, aw["flagged"], KRKi, Kt, aw["pair_R"], aw["pair_t"], aw["pair_aff"], W, H, aw["K4"], 1, float(c["min_act_dist"]))
        act_frame = [0, 1, 2, 3]
        e7, p7, idx = wa.stage7(rec, act_frame)
        assert wu.update(ctx, WID, e7, p7) == 0, ctx.L.sdso_last_error(ctx.h)
        s, maps = wa.sizes_after(win, e7)
        snap = wu.snapshot(ctx, WID, s)
        # ---- the records' integer members, the order and act_index
        ri = out("rec_i", np.int32).reshape(-1, 2)
        assert np.array_equal(ri[:, 0], rec["frame"]) and np.array_equal(ri[:, 1], rec["status"]) and len(idx) > 20
        assert np.array_equal(out("act_index", np.int32), idx)
        ids_p = [p if p >= 0 else win["np"] + (-1 - p) for p in maps[1]]
        ids_r = [q if q >= 0 else win["nr"] + (-1 - q) for q in maps[2]]
        assert list(out("ef_points", np.int32)) == ids_p and list(out("order_points", np.int32)) == maps[1]
        assert list(out("ef_res", np.int32)) == ids_r and list(out("order_res", np.int32)) == maps[2]
        # ---- the window: the activated points' floats came from the device records, not from the driver's zeroed objects
        assert np.array_equal(out("idepth", f32), snap["idepth"], equal_nan=True) and np.abs(snap["idepth"][np.array(maps[1]) < 0]).min() > 0
        assert np.array_equal(out("rstate", np.uint8), snap["res_state"])
        assert np.array_equal(out("energy", np.float64), snap["energy"])
        st = np.concatenate([snap[k].ravel() for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc")])
        assert np.array_equal(out("stitched", np.float64), st, equal_nan=True) and np.nanmax(np.abs(st)) > 0
        assert np.array_equal(out("map", f32).reshape(H >> 1, W >> 1), DC.dm_get(ctx, W, H))
    finally:
        for hid in IDS:
            ctx.L.sdso_imm_release_host(ctx.h, hid)
        for sl in slots:
            ctx.L.sdso_release_pyramid(ctx.h, sl)
        ctx.L.sdso_ba_release_window(ctx.h, WID)
