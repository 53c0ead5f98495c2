"""sdso_shim::WindowedBA::removeOutliers / flagPointsForRemoval (host/sdso_shim.h) driven by host/test_flag_points_shim.cpp on stand-in
types: the device's decisions leave the pointer graph exactly as the reference's two functions do — written out in the driver and
reading the members optimize() wrote back — with writeBackPointStats on and off: pointHessians after each compaction, pointHessiansOut,
pointHessiansMarginalized, every stateFlag, the counters; and the keyframe that goes on from there (dropPointsF, update,
marginalizePointsF) ends in a bit-identical prior.  The window has the size of case A of tests/flag_points_ref.py."""
import numpy as np
import pytest

import flag_points_ref as ref
import shim_driver

ITS = 6


def test_flag_points_driver_compiles():
    """CPU: the two members and their driver compile against the ABI header with the plain host compiler."""
    shim_driver.rebuild("test_flag_points_shim")


def _lists(a, nf):
    """the driver's per-host lists (each behind its length) -> list of lists"""
    out, i = [], 0
    for _ in range(nf):
        n = int(a[i])
        out.append([int(x) for x in a[i + 1:i + 1 + n]])
        i += 1 + n
    assert i == len(a)
    return out


@pytest.mark.gpu
def test_shim_flags_equal_the_reference_functions(tmp_path):
    driver = shim_driver.build("test_flag_points_shim")
    win, frame_marg, _ = ref.make_case("A")
    nf, npts, nr = win["nf"], win["np"], win["nr"]
    n = 8 * nf + 4
    arrays = dict(meta=np.array([nf, npts, nr, win["w"], win["h"], ITS, win["solverMode"]], np.int32),
                  calib=np.concatenate([win["calib_value_scaled"], win["calib_value_zero"]]).astype(np.float64),
                  frame_marg=np.asarray(frame_marg, np.uint8), HM=np.zeros((n, n)), bM=np.zeros(n),
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
    r = shim_driver.run("test_flag_points_shim", tmp_path, arrays)
    print(r.stdout.strip())
    assert driver and len(r.lines) == 3
    # ---- the reference route is not vacuous: every list and every counter moves, points of every fate exist
    cnt = r.out("ref_counters", np.int32)                        # numPointsDropped, flag_oob, flag_in, flag_inin, flag_nores
    assert cnt[0] >= 5 and cnt[3] >= 5 and cnt[2] - cnt[3] >= 5 and cnt[1] - cnt[2] >= 5
    flags = r.out("ref_state_flag", np.int32)
    assert set(flags.tolist()) == {0, 1, 2} and (flags == 1).sum() == cnt[3] and (flags == 2).sum() == cnt[0] + cnt[4] + cnt[1] - cnt[3]
    kept = _lists(r.out("ref_points", np.int32), nf)
    assert sum(len(l) for l in kept) == (flags == 0).sum() and any(l != sorted(l) for l in kept)       # the compaction permutes
    assert any(l != sorted(l) for l in _lists(r.out("ref_ro_points", np.int32), nf))                   # and so does removeOutliers' swap-with-back
    assert np.abs(r.out("ref_HM", np.float64)).max() > 0
    # ---- both shim routes leave what the reference's functions leave
    for tag in ("shim", "nowb"):
        for name in ("ro_points", "ro_out", "points", "out", "marg", "state_flag", "counters", "ef_points"):
            assert np.array_equal(r.out(tag + "_" + name, np.int32), r.out("ref_" + name, np.int32)), (tag, name)
        for name in ("HM", "bM"):
            assert r.out(tag + "_" + name, np.float64).tobytes() == r.out("ref_" + name, np.float64).tobytes(), (tag, name)
