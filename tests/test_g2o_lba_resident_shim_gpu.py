"""sdso_shim::optimizeForkLiveResident and the pair optimizeForkLiveBegin / optimizeForkLiveEnd (host/fork_live.h) driven by
host/test_fork_live_resident_shim.cpp on stand-in types, against the flattened sdso_g2o_lba_optimize_resident call on the same window:
every member of the write-back of FullSystemOptimize.cpp:682-727 is byte-equal to what the C-ABI call's results say, in activeResiduals
order, for the one-call route and for the split one with host work between enqueue and write-back.  The window is that of
tests/test_g2o_lba_shim_gpu.py: case A of tests/g2o_lba_ref.py with its one inactive residual moved to the end of its point's residuals."""
import numpy as np
import pytest

import g2o_lba_ref as ref
import shim_driver


def test_fork_live_resident_driver_compiles():
    """CPU: the shim's three routes and their driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_fork_live_resident_shim")


def _pack(T):
    return np.concatenate([np.asarray(T[0], np.float64).ravel(), np.asarray(T[1], np.float64)])


@pytest.mark.gpu
def test_resident_shim_write_back_equals_the_abi_call(tmp_path, oracle):
    shim_driver.build("test_fork_live_resident_shim")
    c = ref.case("A")
    win = c["win"]
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    res_point, res_target = win["res_point"].copy(), win["res_target"].copy()
    inactive = np.flatnonzero(~ref.reference(oracle, "A")["active"])
    assert len(inactive) == 1
    i0 = int(inactive[0])
    grp = np.flatnonzero(res_point == res_point[i0])
    assert len(grp) >= 2                                            # a point with two residuals whose last one is inactive
    order = np.arange(nr)
    order[grp] = np.concatenate([grp[grp != i0], [i0]])
    res_point, res_target = res_point[order], res_target[order]
    last = int(grp[-1])
    arrays = dict(meta=np.array([nf, npts, nr, win["w"], win["h"], c["iterations"], win["solverMode"]], np.int32),
                  calib=np.concatenate([win["calib_value_scaled"], win["calib_value_zero"]]).astype(np.float64),
                  Twh=np.array([_pack(T) for T in c["Twh"]]), Ttw=np.array([_pack(T) for T in c["Ttw"]]), iterations=np.array([c["iterations"]], np.int32),
                  res_point=res_point.astype(np.int32), res_target=res_target.astype(np.int32))
    for k in ("evalPT", "state", "state_zero"):
        arrays[k] = np.asarray(win[k], np.float64)
    for k in ("ab_exposure", "frameEnergyTH", "u", "v", "idepth", "idepth_zero", "color", "weights"):
        arrays[k] = np.asarray(win[k], np.float32)
    for k in ("frameID", "host"):
        arrays[k] = np.asarray(win[k], np.int32)
    for k in ("hasDepthPrior", "res_state"):
        arrays[k] = np.asarray(win[k], np.uint8)
    for f in range(nf):
        arrays["img%d_l0" % f] = np.asarray(win["pyrs"][f][0], np.float32)
    r = shim_driver.run("test_fork_live_resident_shim", tmp_path, arrays)
    print(r.stdout.strip())
    # ---- the ABI route did something, and the residual moved to the end is the inactive one
    it, stop, n_active = r.out("abi_scalars", np.int32)
    active = r.out("abi_active", np.uint8)
    assert it == 3 and n_active == nr - 1 and active[last] == 0 and active.sum() == nr - 1
    cam, idepth, ih = r.out("abi_cam", np.float64), r.out("abi_idepth", np.float64), r.out("abi_ih", np.float32)
    Twh, aff = r.out("abi_Twh", np.float64).reshape(nf, 12), r.out("abi_aff", np.float64).reshape(nf, 2)
    assert not np.array_equal(Twh, arrays["Twh"]) and not np.array_equal(cam, win["calib_value_scaled"])
    assert idepth[last] == np.float64(win["idepth"][res_point[last]]) and ih[last] == 0
    assert list(r.out("split_done", np.int32))[1] == -4                  # after the fetch there is no job (SDSO_ERR_STATE); the poll before it never waits
    for pre in ("shim", "split"):                                        # optimizeForkLiveResident; optimizeForkLiveBegin / host work / optimizeForkLiveEnd
        # ---- Hcalib, :682-696
        cal = r.out(pre + "_calib", np.float64).reshape(4, 4)
        f32 = cam.astype(np.float32)
        assert np.array_equal(cal[0], cam) and np.array_equal(cal[1], cam) and np.array_equal(cal[2], f32.astype(np.float64))
        assert np.array_equal(cal[3], cam - win["calib_value_zero"])
        assert np.array_equal(r.out(pre + "_calib_i", np.float32), np.array([np.float32(1) / f32[0], np.float32(1) / f32[1], -f32[2] / f32[0], -f32[3] / f32[1]], np.float32))
        # ---- frames, :703-720: every host a residual names
        named = sorted(set(win["host"][res_point].tolist()))
        assert named == list(range(nf))
        sT, sTi, sst = r.out(pre + "_Twh", np.float64).reshape(nf, 12), r.out(pre + "_Thw", np.float64).reshape(nf, 12), r.out(pre + "_state", np.float64).reshape(nf, 4)
        assert np.array_equal(sT, Twh)
        for f in range(nf):
            R, t = Twh[f, :9].reshape(3, 3), Twh[f, 9:]
            Ri = R.T
            ti = -((Ri[:, 0] * t[0] + Ri[:, 1] * t[1]) + Ri[:, 2] * t[2])
            assert np.array_equal(sTi[f, :9].reshape(3, 3), Ri) and np.array_equal(sTi[f, 9:], ti)
        assert np.array_equal(sst[:, 0], aff[:, 0]) and np.array_equal(sst[:, 1], aff[:, 1]) and np.array_equal(sst[:, 2:], sst[:, :2])
        # ---- residuals, :722-723 and the members applyRes reads
        assert np.array_equal(r.out(pre + "_cpt", np.float32), r.out("abi_cpt", np.float32))
        assert np.array_equal(r.out(pre + "_energy", np.float64), r.out("abi_energy", np.float32).astype(np.float64))
        assert np.array_equal(r.out(pre + "_newstate", np.uint8), r.out("abi_state", np.uint8))
        # ---- points, :724-726, in activeResiduals order
        pts = r.out(pre + "_points", np.float32).reshape(npts, 5)          # idepth idepth_scaled idepth_zero idepth_hessian HdiF
        want = np.zeros((npts, 5), np.float32)
        want[:, 0] = want[:, 1] = win["idepth"]; want[:, 2] = win["idepth_zero"]; want[:, 3] = 7.0
        for k in range(nr):
            p = res_point[k]
            want[p, 0:3] = np.float32(idepth[k])
            if ih[k] != 0:
                want[p, 3] = ih[k]
            want[p, 4] = np.float32(1.0 / np.float64(want[p, 3]))
        assert np.array_equal(pts, want)
        p0 = res_point[last]
        assert pts[p0, 0] == win["idepth"][p0] and np.float32(idepth[grp[0]]) != win["idepth"][p0]      # the inactive last residual won
        assert (pts[:, 3] != 7.0).sum() > 100
        assert r.out(pre + "_rmse", np.float32)[0] == r.out("abi_rmse", np.float32)[0] > 0
