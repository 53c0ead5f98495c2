"""sdso_shim::WindowedBA::update (host/sdso_shim.h) driven by host/test_window_update.cpp on stand-in types: one keyframe step (optimize,
the toRemove drops, removeOutliers, update instead of a second upload) leaves the device window the C-ABI path from Python leaves
(tests/test_ba_window_update_gpu.py::test_update_after_optimize_equals_fresh_upload's edit), bit for bit, and the EnergyFunctional's
own lists in the order of the Python model."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import shim_driver
import synth
import window_edit_ref as ref
import window_update_helpers as wu

ITS = 6


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_window_update")


def test_window_update_driver_compiles():
    """CPU: WindowedBA::update and its driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_window_update")


def _first_frames(big, nfw):
    """the window of the first nfw frames of `big`: their points, the residuals among them"""
    pts = np.nonzero(big["host"] < nfw)[0]
    pmap = -np.ones(big["np"], np.int64); pmap[pts] = np.arange(len(pts))
    rk = np.nonzero((pmap[big["res_point"]] >= 0) & (big["res_target"] < nfw))[0]
    w = dict(big)
    w.update(nf=nfw, np=len(pts), nr=len(rk))
    for k in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID"):
        w[k] = np.ascontiguousarray(big[k][:nfw])
    w["pyrs"] = big["pyrs"][:nfw]
    for k in ("u", "v", "idepth", "idepth_zero", "color", "weights", "host", "hasDepthPrior"):
        w[k] = np.ascontiguousarray(big[k][pts])
    w["res_point"] = pmap[big["res_point"][rk]].astype(np.int32); w["res_target"] = np.ascontiguousarray(big["res_target"][rk])
    w["res_state"] = np.zeros(len(rk), np.uint8)
    n = 8 * nfw + 4
    w["HM"] = np.zeros((n, n)); w["bM"] = np.zeros(n)
    return w, pts


@pytest.mark.gpu
def test_shim_update_equals_the_abi_path(gpu_ctx, driver, tmp_path):
    """Three steps (host/test_window_update.cpp): the edit after optimize; a frame, residuals and points inserted (the window grows from 5 to
    6 frames); marginalizePointsF on the grown window, the removePoint loop, WindowedBA::marginalizeFrame and the update that follows."""
    ctx = gpu_ctx
    big = synth.ba_window(w=640, h=480, nf=6, pts_per_kf=150, seed=5207, idepth_noise=0.1, max_res_per_point=8)
    win, in_win = _first_frames(big, 5)
    held = np.zeros(win["np"], bool); held[np.random.RandomState(3).permutation(win["np"])[:60]] = True     # inserted in step 2
    keep_p = np.nonzero(~held)[0]
    pm = -np.ones(win["np"], np.int64); pm[keep_p] = np.arange(len(keep_p))
    full = win
    win = dict(full)
    rk = pm[full["res_point"]] >= 0
    for k in ("u", "v", "idepth", "idepth_zero", "color", "weights", "host", "hasDepthPrior"):
        win[k] = np.ascontiguousarray(full[k][keep_p])
    win["res_point"] = pm[full["res_point"][rk]].astype(np.int32); win["res_target"] = np.ascontiguousarray(full["res_target"][rk])
    win["res_state"] = np.zeros(int(rk.sum()), np.uint8); win["np"] = len(keep_p); win["nr"] = int(rk.sum())
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    arrays = dict(meta=np.array([nf, npts, nr, win["w"], win["h"], ITS, win["solverMode"], big["nf"]], np.int32),
                  calib=np.concatenate([win["calib_value_scaled"], win["calib_value_zero"]]).astype(np.float64))
    for k in ("evalPT", "state", "state_zero"):
        arrays[k] = np.asarray(big[k], np.float64)
    for k in ("ab_exposure", "frameEnergyTH"):
        arrays[k] = np.asarray(big[k], np.float32)
    arrays["frameID"] = np.asarray(big["frameID"], np.int32)
    for k in ("u", "v", "idepth", "idepth_zero", "color", "weights"):
        arrays[k] = np.asarray(win[k], np.float32)
    for k in ("res_point", "res_target", "host"):
        arrays[k] = np.asarray(win[k], np.int32)
    for k in ("hasDepthPrior", "res_state"):
        arrays[k] = np.asarray(win[k], np.uint8)
    for f in range(big["nf"]):
        arrays["img%d_l0" % f] = np.asarray(big["pyrs"][f][0], np.float32)
    # ---- step 1 through the C-ABI
    wu.upload_pyramids(ctx, big)
    wu.upload(ctx, win, 3)
    wu.optimize(ctx, 3, ITS)
    d = wu.post_state(ctx, 3, win)
    edit = wu.outlier_edit(win, d)
    assert len(edit["drop_res"]) > 0 and edit["drop_point"].sum() > 0
    w1, maps1 = wu.flatten(win, wu.values_from_post(win, d), edit, {})
    assert wu.update(ctx, 3, edit) == 0, ctx.L.sdso_last_error(ctx.h)
    s1 = wu.snapshot(ctx, 3, w1)
    ids_p = [int(p) for p in maps1[1]]; ids_r = [int(r) for r in maps1[2]]           # ids of the uploaded window, as the driver numbers them
    # ---- step 2: frame 5 comes; the points of the two newest hosts observe it; the held-back points enter with a residual into every other frame
    hp = np.nonzero(held)[0]
    add_res = [(p, nf) for p in range(w1["np"]) if w1["host"][p] >= nf - 2]
    hosts = [int(full["host"][p]) for p in hp]
    pt_res = [(q, t) for q, h in enumerate(hosts) for t in range(nf + 1) if t != h]
    edit2 = dict(n_add_frames=1, add_res=add_res, add_points=hosts, pt_res=pt_res)
    payload2 = dict(add_frames={k: np.ascontiguousarray(big[k][nf:nf + 1]) for k in ("evalPT", "state", "state_zero", "ab_exposure", "frameEnergyTH", "frameID")},
                    add_points={k: np.ascontiguousarray(full[k][hp]) for k in ("u", "v", "idepth", "idepth_zero", "color", "weights", "hasDepthPrior")})
    payload2["add_frames"]["pyrs"] = [big["pyrs"][nf]]
    arrays.update(s2_add_res_point=np.array([ids_p[p] for p, _ in add_res], np.int32), s2_pt_host=np.array(hosts, np.int32),
                  s2_pr_point=np.array([q for q, _ in pt_res], np.int32), s2_pr_target=np.array([t for _, t in pt_res], np.int32),
                  s2_pt_u=full["u"][hp], s2_pt_v=full["v"][hp], s2_pt_idepth=full["idepth"][hp], s2_pt_color=full["color"][hp], s2_pt_weights=full["weights"][hp])
    vals1 = wu.values_from_state(ctx, 3, w1)
    w2, maps2 = wu.flatten(w1, vals1, edit2, payload2)
    assert wu.update(ctx, 3, edit2, payload2) == 0, ctx.L.sdso_last_error(ctx.h)
    n_ar = len(add_res)
    ids_p2 = [ids_p[p] if p >= 0 else npts + (-1 - p) for p in maps2[1]]
    ids_r2 = [ids_r[r] if r >= 0 else nr + (-1 - r) for r in maps2[2]]
    # ---- step 3: every point of the oldest frame and a seeded part of the others is marginalised, the frame leaves
    flags = ((w2["host"] == 0) | (np.random.RandomState(8).rand(w2["np"]) < 0.06)).astype(np.uint8)
    arrays["s3_marg"] = np.array([ids_p2[p] for p in np.nonzero(flags)[0]], np.int32)
    r = shim_driver.run("test_window_update", tmp_path, arrays)
    print(r.stdout.strip())
    mp = wu.marginalize_points(ctx, 3, w2, flags)
    mf = wu.marginalize_frame_dev(ctx, 3, 0, w2["nf"] - 1)
    edit3 = dict(remove_points=[int(p) for p in np.nonzero(flags)[0]], remove_frames=[0])
    maps3 = ref.apply_edit(w2["nf"], w2["host"], w2["res_point"], w2["res_target"], edit3)
    assert wu.update(ctx, 3, edit3) == 0, ctx.L.sdso_last_error(ctx.h)
    ids_p3 = [ids_p2[p] for p in maps3[1]]; ids_r3 = [ids_r2[r] for r in maps3[2]]
    s3 = wu.snapshot(ctx, 3, dict(nf=len(maps3[0]), np=len(maps3[1]), nr=len(maps3[2])))
    # ---- step 1: the EnergyFunctional after dropResidual / dropPointsF, the device's maps and the model agree; the window computes the same
    assert list(r.out("ef_points", np.int32)) == ids_p == list(r.out("order_points", np.int32))
    assert list(r.out("ef_res", np.int32)) == ids_r == list(r.out("order_res", np.int32))

    def same(prefix, s):
        assert np.array_equal(r.out(prefix + "idepth", np.float32), s["idepth"])
        assert np.array_equal(r.out(prefix + "rstate", np.uint8), s["res_state"])
        assert np.array_equal(r.out(prefix + "energy", np.float64), s["energy"])
        st = np.concatenate([s[k].ravel() for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc")])
        assert np.array_equal(r.out(prefix + "stitched", np.float64), st) and np.abs(st).max() > 0
    assert np.array_equal(r.out("state", np.float64), s1["state"].ravel())
    same("", s1)
    # ---- step 2: the grown window's order
    assert list(r.out("s2_ef_points", np.int32)) == ids_p2 and list(r.out("s2_ef_res", np.int32)) == ids_r2
    assert len(maps2[0]) == nf + 1 and n_ar > 0 and len(hosts) > 0
    # ---- step 3: the prior after marginalizePointsF (6 frames: 52 x 52) and after marginalizeFrame (44 x 44), the window that is left
    assert np.array_equal(r.out("s3_HM", np.float64), mp[0].ravel()) and np.array_equal(r.out("s3_bM", np.float64), mp[1])
    assert mp[0].shape == (52, 52) and np.abs(mp[0]).max() > 0
    assert np.array_equal(r.out("s3_HMf", np.float64), mf[0].ravel()) and np.array_equal(r.out("s3_bMf", np.float64), mf[1])
    assert list(r.out("s3_ef_points", np.int32)) == ids_p3 and list(r.out("s3_ef_res", np.int32)) == ids_r3
    same("s3_", s3)
    ctx.check(ctx.L.sdso_ba_release_window(ctx.h, 3))
