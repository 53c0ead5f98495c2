"""sdso_shim::CoarseDistanceMap / selectPointsToActivate (host/sdso_shim.h) driven by host/test_distmap_shim.cpp on stand-in types:
what the program finds in its objects equals the C-ABI path from Python on the same inputs, exactly."""

import numpy as np
import pytest

import distmap_cases as Cs
import distmap_ref as R
import shim_driver
import synth

f32 = np.float32


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_distmap_shim")


def test_distmap_shim_driver_compiles():
    """CPU: the shim's new members + the driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_distmap_shim")


@pytest.mark.gpu
def test_shim_distance_map_and_selection(gpu_ctx, driver, tmp_path):
    w, h, nhost = 1232, 368, 7
    case = Cs.selection_case(w=w, h=h, nhost=nhost, per_host=900, n_active=2000, min_act_dist=1.5, seed=41)
    a, c = case["active"], case["cand"]
    # poses of the nhost + 1 keyframes (the newest last) and their inverses, as FrameHessian::PRE_worldToCam / PRE_camToWorld
    rs = np.random.RandomState(8)
    w2c, c2w = [], []
    for k in range(nhost + 1):
        xi = np.array([0, 0, -0.2 * k, 0, 0, 0], np.float64)
        xi[3:] = rs.normal(0, 0.01, 3); xi[0:2] = rs.normal(0, 0.02, 2)
        T = synth.se3_exp(xi)
        w2c.append(synth.se3_pack(T)); c2w.append(synth.se3_pack(synth.se3_inv(T)))
    cal = synth.kitti_calib(w, h)
    add = np.array([[300, 90], [301, 90], [10, 10], [0, 5], [615, 100], [400, 183]], np.int32)
    arrays = dict(meta=np.array([w, h, synth.pyramid_levels(w, h), nhost + 1], np.int32), calib=np.array([cal["fx"], cal["fy"], cal["cx"], cal["cy"]], f32),
                  worldToCam=np.array(w2c, np.float64), camToWorld=np.array(c2w, np.float64), flagged=case["flagged"],
                  a_host=a["pg"], a_u=a["u"], a_v=a["v"], a_idepth=a["idepth"],
                  c_host=c["pg"], c_status=c["status"].astype(np.int32), c_u=c["u"], c_v=c["v"], c_idepth_min=c["idepth_min"], c_idepth_max=c["idepth_max"],
                  c_quality=c["quality"], c_interval=c["interval"], c_my_type=c["my_type"],
                  par=np.array([case["min_act_dist"], case["min_trace_quality"]], f32), add=add)
    r = shim_driver.run("test_distmap_shim", tmp_path, arrays, mode="run")
    head, out = r.stdout.split(), r.out
    # the geometries the shim formed (K[1] * R * Ki[0], K[1] * t in float) are the caller's side of the C-ABI: the same values go
    # through it from here; they are the float products of the double poses up to the rounding of the order of operations
    g = out("geoms", f32).reshape(nhost, 12)
    KRKi, Kt = g[:, :9].reshape(nhost, 3, 3), g[:, 9:]
    KRKi_py, Kt_py = Cs.window_geoms(np.array(w2c), (cal["fx"], cal["fy"], cal["cx"], cal["cy"]))
    assert np.allclose(KRKi, KRKi_py, rtol=1e-4, atol=1e-4) and np.allclose(Kt, Kt_py, rtol=1e-4, atol=1e-4)
    case["KRKi"], case["Kt"] = KRKi, Kt
    h1, w1 = h >> 1, w >> 1
    n_seeds = Cs.dm_make(gpu_ctx, w, h, KRKi, Kt, a["pg"], a["u"], a["v"], a["idepth"])
    map0 = Cs.dm_get(gpu_ctx, w, h)
    assert int(head[1]) == n_seeds and n_seeds > 1500
    assert np.array_equal(out("map0", f32).reshape(h1, w1), map0)
    Cs.dm_add(gpu_ctx, add[:, 0], add[:, 1])
    map1 = Cs.dm_get(gpu_ctx, w, h)
    assert np.array_equal(out("map1", f32).reshape(h1, w1), map1) and (map1 < map0).any()
    Cs.dm_make(gpu_ctx, w, h, KRKi, Kt, a["pg"], a["u"], a["v"], a["idepth"])
    got = Cs.dm_select(gpu_ctx, case)
    dec = out("decision", np.uint8)
    assert np.array_equal(dec, got["decision"]) and int(head[3]) == got["n_selected"]
    assert np.array_equal(out("order", np.int32), np.nonzero(got["decision"] == 2)[0])       # toOptimize in the reference's loop order
    assert np.array_equal(out("map2", f32).reshape(h1, w1), Cs.dm_get(gpu_ctx, w, h))
    assert min((dec == k).sum() for k in (0, 1, 2)) > 100
    # and both are what the CPU statement gives
    _, _, m = R.make_distance_map(w, h, KRKi, Kt, a["pg"], a["u"], a["v"], a["idepth"])
    assert np.array_equal(Cs.ref_select(R, case, m)["decision"], dec)
