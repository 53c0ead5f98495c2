"""GPU parity of the BA linearisation on a window that takes EVERY exit of PointFrameResidual::linearize (tests/lin_exits_cases.py;
tests/test_lin_exits_ref.py asserts on the oracle that it does: IN 232, OUTLIER 267, OOB 128 = 57 preset-sticky + 49 `drescale <= 0`
+ 7 centre + 15 pattern pixel).  The exits are `return`s in linearize_one and the `dead` flag in linearize_coop (csrc/ba_lin.hip); both
expand the same statements.

The window goes through three paths, as in tests/test_ba_tiles_gpu.py — the fused batch path (a batch of one) with the Jacobian records and
without them, and the un-fused `sdso_ba_linearize` + `sdso_ba_apply_res` — for two rounds of linearize + applyRes each.  Round 1
meets the preset-sticky residuals (the upload carries `res_state = 1`) and every fresh exit; in round 2 all 128 OOB residuals of round 1
are sticky; the un-fused path runs it at the newest frame's new threshold (IN 232 -> 325), the batch
phase at the uploaded ones.  After each round everything the linearisation decides is compared bit for bit with the oracle's same round: ns, ne, nw, st,
act, JpJdF of the active residuals, and with records Je of the active and Jn of the OUTLIER residuals.
"""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import lin_exits_cases as Lx
from test_ba_tiles_gpu import _readback

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(oracle):
    win = Lx.window()
    return win, {True: Lx.oracle_rounds(oracle, win), False: Lx.oracle_rounds(oracle, win, new_frame_th=False)}


def _compare(o, g, records):
    assert np.array_equal(o["ns"], g["ns"]) and np.array_equal(o["ne"], g["ne"]) and np.array_equal(o["nw"], g["nw"])
    assert np.array_equal(o["st"], g["st"]) and np.array_equal(o["act"], g["act"])
    act, outl = o["act"] == 1, o["ns"] == 2
    assert act.sum() > 200 and outl.sum() > 100 and (o["ns"] == 1).sum() >= 128      # the comparison is not vacuous
    assert np.array_equal(o["jp"][act], g["jp"][act])
    if records:
        assert np.array_equal(o["Je"][act], g["Je"][act])
        assert np.array_equal(o["Jn"][outl], g["Jn"][outl])


@pytest.mark.parametrize("path", ["fused_records", "fused_registers", "unfused"])
def test_every_exit_matches_oracle(gpu_ctx, case, path):
    ctx = gpu_ctx
    win, rounds = case[0], case[1][path == "unfused"]                 # (which thresholds round 2 runs at: lin_exits_cases.oracle_rounds)
    wid, slots = 91, [910 + f for f in range(win["nf"])]
    for f in range(win["nf"]):
        ctx.upload_pyramid(slots[f], win["pyrs"][f][:1])              # level 0 only
    Wd, keep = abi.make_ba_window(win, frame_slots=slots, dI_list=[p[0] for p in win["pyrs"]])
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid, C.byref(Wd)))
    try:
        records = path != "fused_registers"
        if path != "unfused":
            ctx.check(ctx.L.sdso_ba_batch_create(ctx.h, 1, abi.ip(np.array([wid], np.int32))))
            ctx.check(ctx.L.sdso_ba_batch_set_materialize(ctx.h, int(records)))
        for rnd, o in enumerate(rounds):
            if path == "unfused":
                ctx.check(ctx.L.sdso_ba_linearize(ctx.h, wid, None))
                g = _readback(ctx, win, wid, True, lin_only=True)       # PointFrameResidual::J before applyRes swaps it, as the oracle reads it
                ctx.check(ctx.L.sdso_ba_apply_res(ctx.h, wid))
                g2 = _readback(ctx, win, wid, True)
                for k in ("Je", "st", "act", "jp"):
                    g[k] = g2[k]
            else:
                ctx.check(ctx.L.sdso_ba_batch_accumulate(ctx.h))
                g = _readback(ctx, win, wid, records)
            print("%s round %d: IN %d OUTLIER %d OOB %d" % (path, rnd + 1, (g["ns"] == 0).sum(), (g["ns"] == 2).sum(), (g["ns"] == 1).sum()))
            _compare(o, g, records)
    finally:
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, wid))
