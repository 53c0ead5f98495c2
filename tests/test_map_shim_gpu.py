"""sdso_shim::PointMap / KeyFrameDisplay (host/sdso_shim.h) driven by host/test_map_shim.cpp on stand-in types: the route through the shim
leaves the same lists, vertices, colours and refreshPC return values as KeyFrameDisplay::setFromKF / refreshPC written out in the driver
over the members optimize() wrote back — on window A of tests/flag_points_ref.py through one keyframe, with an immature group on one
frame, across a changed and an unchanged setting, and in the many-frames form.  sparsity = 2 throws."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import flag_points_ref as fref
import map_ref as ref
import shim_driver

ITS = 6


def test_map_driver_compiles():
    """CPU: the two classes and their driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_map_shim")


def _oracle_thresholds(oracle, win, frame_marg, last_gone):
    """the quantile thresholds of tests/map_ref.py on the CPU oracle's post-state: numbers both routes are handed"""
    W, keep = abi.make_ba_window(win, dI_list=[p[0] for p in win["pyrs"]])
    h = oracle.orc_ba_create(C.byref(W))
    res = abi.BAOptResult()
    oracle.orc_ba_optimize(h, ITS, None, None, None, C.byref(res))
    P, post = abi.make_post_state(win["nf"], win["np"], win["nr"])
    oracle.orc_ba_get_post_state(h, C.byref(P))
    oracle.orc_ba_destroy(h)
    th = ref.quantile_thresholds(ref.case_on_post("A", win, post, frame_marg, last_gone)["frames"])
    return np.array([th["scaledTH"], th["absTH"], th["minBS"]], np.float32)


@pytest.mark.gpu
def test_shim_map_equals_the_reference_functions(tmp_path, oracle):
    driver = shim_driver.build("test_map_shim")
    win, frame_marg, last_gone = fref.make_case("A")
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    n = 8 * nf + 4
    arrays = dict(meta=np.array([nf, npts, nr, win["w"], win["h"], ITS, win["solverMode"]], np.int32),
                  calib=np.concatenate([win["calib_value_scaled"], win["calib_value_zero"]]).astype(np.float64),
                  frame_marg=np.asarray(frame_marg, np.uint8), HM=np.zeros((n, n)), bM=np.zeros(n), th=_oracle_thresholds(oracle, win, frame_marg, last_gone),
                  maxRelBaseline=np.zeros(npts, np.float32), numGoodResiduals=np.asarray(win["numGoodResiduals"], np.int32), res_isNew=np.ones(nr, np.uint8))
    for k in ("evalPT", "state", "state_zero"):
        arrays[k] = np.asarray(win[k], np.float64)
    for k in ("ab_exposure", "frameEnergyTH", "u", "v", "idepth", "idepth_zero", "color", "weights"):
        arrays[k] = np.asarray(win[k], np.float32)
    for k in ("frameID", "res_point", "res_target", "host"):
        arrays[k] = np.asarray(win[k], np.int32)
    for k in ("hasDepthPrior", "res_state"):
        arrays[k] = np.asarray(win[k], np.uint8)
    for f in range(nf):
        arrays["img%d_l0" % f] = np.asarray(win["pyrs"][f][0], np.float32)
    r = shim_driver.run("test_map_shim", tmp_path, arrays)
    print(r.stdout.strip())
    assert driver and "sparsity 2 refused" in r.lines and "refused refresh kept needRefresh" in r.lines
    # ---- the reference route is not vacuous
    counts = r.out("ref_counts", np.int32).reshape(3, nf)
    assert counts.sum() == npts and counts.sum(1).min() >= 50
    rets = r.out("ref_rets", np.int32)
    per = rets[:5 * nf].reshape(nf, 5)                            # new settings, unchanged, canRefresh = false, changed, id
    assert (per[:, 0] == 1).all() and (per[:, 1] == 0).all() and (per[:, 2] == 0).all() and (per[:, 3] == 1).all()
    assert per[:, 4].tolist() == [100 + f for f in range(nf)] and (rets[5 * nf:] == 1).all()
    good = r.out("ref_good", np.int32)
    g14 = good[:2 * nf].reshape(nf, 2)
    assert (g14[:, 0] > 0).sum() >= nf // 2 and g14[:, 1].sum() > g14[:, 0].sum() >= 8 * 50
    assert g14[1, 1] >= 8 * 13                                    # mode 0 at minBS = 0 shows the untraced immature points: 13 x 8 NaN vertices
    v4 = r.out("ref_v4", np.float32)
    assert np.isnan(v4).sum() == 3 * 8 * 13 and len(r.out("ref_v1", np.float32)) == 3 * g14[:, 0].sum()
    # ---- the two routes leave identical dumps
    for name, dt in (("counts", np.int32), ("list1", np.uint32), ("list2", np.uint32), ("list3", np.uint32), ("rets", np.int32), ("good", np.int32),
                     ("v1", np.uint32), ("c1", np.uint8), ("v4", np.uint32), ("c4", np.uint8), ("vm", np.uint32), ("cm", np.uint8)):
        a, b = r.out("ref_" + name, dt), r.out("shim_" + name, dt)
        if name in ("v4",):                                       # a NaN vertex: NaN in the same place
            fa, fb = a.view(np.float32), b.view(np.float32)
            assert np.array_equal(np.isnan(fa), np.isnan(fb)), name
            a, b = a[~np.isnan(fa)], b[~np.isnan(fb)]
        assert len(a) > 0 and np.array_equal(a, b), (name, len(a), len(b))
