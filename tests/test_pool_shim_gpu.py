"""The threaded binding of INTEGRATION.md §2 with a device buffer pool, through the shim (host/test_pool_shim.cpp on stand-in types): the
schedule of tests/test_handoff_shim_gpu.py — a mapping thread on one sdso_shim::Device builds and exports a tracking template and three
frames per keyframe, a tracking thread on a second Device adopts and imports them — with ONE sdso_shim::Pool attached to both Devices
(Device::setPool).  The buffers of every keyframe are the ones an earlier keyframe left behind, while the other thread may still be at
work on them; the program compares with the same schedule on one Device in one thread WITHOUT a pool: every pose, affine pair, residual
and iteration count must be bit-equal, and the pool must not have made a single host wait.

Six independent 320 x 240 windows (tracking_ref_window_cases.make_case, seeds 3101 + k), 3 optimisation steps each."""
import os

import numpy as np
import pytest

import shim_driver
import tracking_ref_window_cases as TC
from test_handoff_shim_gpu import _arrays, K, ITS, TRACKED, REC, NF


@pytest.fixture(scope="module")
def driver():
    return shim_driver.build("test_pool_shim")


def test_pool_shim_driver_compiles():
    """CPU: sdso_shim::Pool, Device::setPool and the driver compile against the ABI header with the host compiler."""
    shim_driver.rebuild("test_pool_shim")


@pytest.mark.gpu
def test_pooled_two_threads_equal_unpooled_one(driver, tmp_path):
    cases = [dict(nf=NF, pts_per_kf=200, seed=3101 + k) for k in range(K)]
    arrays = dict(meta=np.array([K, NF, ITS], np.int32))
    for k, case in enumerate(TC.make_case(**spec) for spec in cases):
        os.makedirs(str(tmp_path / ("k%d" % k)))
        for name, a in _arrays(case).items():
            arrays["k%d/%s" % (k, name)] = a
    r = shim_driver.run("test_pool_shim", tmp_path, arrays, timeout=60)
    print(r.stdout)
    assert "pool ok" in r.stdout
    two, one = r.out("two", np.float64).reshape(K * TRACKED, REC), r.out("one", np.float64).reshape(K * TRACKED, REC)
    assert two.tobytes() == one.tobytes()                                 # poses, affine pairs, lastResiduals, iteration counts
    assert (two[:, 19:24].sum(axis=1) > 0).all() and np.isfinite(two[:, :14]).all()               # every frame was iterated on
    hits, misses, frees, host_waits, overflow_waits, parked, parked_bytes = r.out("stats", np.float64)
    assert host_waits == 0 and overflow_waits == 0 and hits > 0 and misses == frees + parked
