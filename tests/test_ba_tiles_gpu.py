"""GPU parity of the BA linearisation on the tiled level-0 image (12-byte pixels in 5x2 tiles, csrc/tile0_layout.h) at image sizes that
exercise the tile geometry: widths 161..165 (every residue modulo 5), odd and even heights, level 0 only.

Five windows, `synth.ba_window(w, h, nf=4, pts_per_kf=60, seed=3100 + w)`.  The oracle on these inputs (asserted below):

    window      residuals IN   of
    (161, 97)   353            649
    (162, 97)   345            622
    (163, 98)   321            627
    (164, 99)   350            617
    (165, 97)   335            605

the rest OUTLIER, none OOB, so `(ns == 0).sum() > 0.4 * nr` holds on every one (0.51-0.57).  Each window goes through three paths —
the fused batch path (`sdso_ba_batch_accumulate`, a batch of one) with the Jacobian records and without them, and the unfused
`sdso_ba_linearize` + `sdso_ba_apply_res` — and everything the linearisation decides is compared bit for bit with the oracle:
ns, ne, nw, st, act, JpJdF of the active residuals, and with records Je of the active and Jn of the OUTLIER residuals.

One batch of 11 windows of the (163, 98) shape (more than 8 and not a multiple of 8 — the fused kernel deals the windows of a batch
to the eight XCDs in groups of eight) pins the launch shape: a window or a chunk that is skipped or visited twice shows in that
window's comparison.

Border coverage.  The linearisation accepts a pattern pixel at Ku < w - 3, Kv < h - 3, but synth.ba_window admits a residual only
where the pattern's centre projects to 8 < u < w - 9, 8 < v < h - 9 (at the true depth), so with the pattern's reach of 2 pixels and
the bilinear tap's +1 the last pixel a tap of these windows reaches is x = w - 7, y = h - 7: tile column (w - 7) // 5, tile row
(h - 7) >> 1.  `_border_taps` counts, in numpy from the window's poses, intrinsics and idepths, the linearised residuals with a tap
in that tile column and in that tile row (or beyond: the idepth noise moves a few projections further out); each window must have
at least one of each kind.  With the seeds above the counts are (column / row) 9 / 3, 3 / 5, 6 / 6, 11 / 2 and 5 / 2, so no seed had
to be changed.
"""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import synth

pytestmark = pytest.mark.gpu

SIZES = [(161, 97), (162, 97), (163, 98), (164, 99), (165, 97)]
ORACLE_IN = {(161, 97): (353, 649), (162, 97): (345, 622), (163, 98): (321, 627), (164, 99): (350, 617), (165, 97): (335, 605)}
NBATCH = 11
BATCH_SEEDS = [4100 + 13 * k for k in range(NBATCH)]


def _oracle_lin(oracle, win, W):
    nr = win["nr"]
    h = oracle.orc_ba_create(C.byref(W))
    o = dict(Jn=np.zeros((nr, 74), np.float32), ns=np.zeros(nr, np.uint8), ne=np.zeros(nr, np.float32), nw=np.zeros(nr, np.float32),
             Je=np.zeros((nr, 74), np.float32), st=np.zeros(nr, np.uint8), act=np.zeros(nr, np.uint8), jp=np.zeros((nr, 8), np.float32))
    oracle.orc_ba_linearize(h, None)
    oracle.orc_ba_get_linearization(h, abi.fp(o["Jn"]), abi.bp(o["ns"]), abi.fp(o["ne"]), abi.fp(o["nw"]), None, None)
    oracle.orc_ba_apply_res(h)
    oracle.orc_ba_get_ef_jacobians(h, abi.fp(o["Je"]))
    oracle.orc_ba_get_residual_state(h, abi.bp(o["st"]), abi.bp(o["act"]), abi.fp(o["jp"]))
    oracle.orc_ba_destroy(h)
    for a in o.values():
        a.setflags(write=False)
    return o


def _case(oracle, w, h, seed):
    win = synth.ba_window(w, h, nf=4, pts_per_kf=60, seed=seed)
    W, keep = abi.make_ba_window(win, dI_list=[p[0] for p in win["pyrs"]])
    return dict(win=win, o=_oracle_lin(oracle, win, W))


@pytest.fixture(scope="module")
def cases(oracle):
    return {(w, h): _case(oracle, w, h, 3100 + w) for (w, h) in SIZES}


@pytest.fixture(scope="module")
def batch_cases(oracle):
    return [_case(oracle, 163, 98, s) for s in BATCH_SEEDS]


def _border_taps(win, ns):
    """(residuals with a tap in tile column >= (w - 7) // 5, residuals with a tap in tile row >= (h - 7) >> 1) among the linearised ones"""
    w, h = win["w"], win["h"]
    fx, fy, cx, cy = [np.float64(v) for v in win["K"]]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    Ki = np.linalg.inv(K)
    pt, tg = np.asarray(win["res_point"]), np.asarray(win["res_target"])
    host = np.asarray(win["host"])[pt]
    u, v, idp = [np.asarray(win[k], np.float64)[pt] for k in ("u", "v", "idepth")]
    col = np.zeros(len(pt), bool)
    row = np.zeros(len(pt), bool)
    for i in range(len(pt)):
        R, t = synth.se3_mul(win["poses"][tg[i]], synth.se3_inv(win["poses"][host[i]]))
        KRKi, Kt = K @ R @ Ki, K @ t
        for dx, dy in synth.PATTERN:
            q = KRKi @ np.array([u[i] + dx, v[i] + dy, 1.0]) + Kt * idp[i]
            x1, y1 = int(q[0] / q[2]) + 1, int(q[1] / q[2]) + 1        # the far corner of the bilinear tap
            col[i] |= x1 // 5 >= (w - 7) // 5
            row[i] |= (y1 >> 1) >= (h - 7) >> 1
    lin = np.asarray(ns) != 1
    return int((col & lin).sum()), int((row & lin).sum())


def _upload(ctx, case, wid, slot0):
    win = case["win"]
    slots = [slot0 + f for f in range(win["nf"])]
    for f in range(win["nf"]):
        ctx.upload_pyramid(slots[f], win["pyrs"][f][:1])              # level 0 only
    W, keep = abi.make_ba_window(win, frame_slots=slots, dI_list=[p[0] for p in win["pyrs"]])
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid, C.byref(W)))
    return W, keep


def _readback(ctx, win, wid, records, lin_only=False):
    nr = win["nr"]
    g = dict(Jn=np.zeros((nr, 74), np.float32), ns=np.zeros(nr, np.uint8), ne=np.zeros(nr, np.float32), nw=np.zeros(nr, np.float32),
             Je=np.zeros((nr, 74), np.float32), st=np.zeros(nr, np.uint8), act=np.zeros(nr, np.uint8), jp=np.zeros((nr, 8), np.float32))
    ctx.check(ctx.L.sdso_ba_get_linearization(ctx.h, wid, abi.fp(g["Jn"]) if records else None, abi.bp(g["ns"]), abi.fp(g["ne"]), abi.fp(g["nw"]), None, None))
    if lin_only:
        return g
    if records:
        ctx.check(ctx.L.sdso_ba_get_ef_jacobians(ctx.h, wid, abi.fp(g["Je"])))
    ctx.check(ctx.L.sdso_ba_get_residual_state(ctx.h, wid, abi.bp(g["st"]), abi.bp(g["act"]), abi.fp(g["jp"])))
    return g


def _compare(o, g, nr, records):
    assert (o["ns"] == 0).sum() > 0.4 * nr                                            # the comparison is not vacuous
    # linearize: decisions and energies of every residual
    assert np.array_equal(o["ns"], g["ns"]) and np.array_equal(o["ne"], g["ne"]) and np.array_equal(o["nw"], g["nw"])
    # applyRes: states, isActive, JpJdF
    assert np.array_equal(o["st"], g["st"]) and np.array_equal(o["act"], g["act"])
    act = o["act"] == 1
    assert act.sum() > 0
    assert np.array_equal(o["jp"][act], g["jp"][act])
    if records:
        assert np.array_equal(o["Je"][act], g["Je"][act])
        outl = o["ns"] == 2
        assert outl.sum() > 0
        assert np.array_equal(o["Jn"][outl], g["Jn"][outl])


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_oracle_counts_and_border_coverage(cases, size):
    win, o = cases[size]["win"], cases[size]["o"]
    n_in, n_all = ORACLE_IN[size]
    assert win["nr"] == n_all and (o["ns"] == 0).sum() == n_in and (o["ns"] == 2).sum() == n_all - n_in and (o["ns"] == 1).sum() == 0
    ncol, nrow = _border_taps(win, o["ns"])
    print("window %s: residuals with a tap in the last reachable tile column %d, tile row %d" % (size, ncol, nrow))
    assert ncol >= 1 and nrow >= 1


@pytest.mark.parametrize("path", ["fused_records", "fused_registers", "unfused"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_tiled_linearisation_matches_oracle(gpu_ctx, cases, size, path):
    ctx = gpu_ctx
    case = cases[size]
    win, o = case["win"], case["o"]
    wid = 90
    W, keep = _upload(ctx, case, wid, 900)
    try:
        if path == "unfused":
            ctx.check(ctx.L.sdso_ba_linearize(ctx.h, wid, None))
            g = _readback(ctx, win, wid, True, lin_only=True)           # PointFrameResidual::J before applyRes swaps it, as the oracle reads it
            ctx.check(ctx.L.sdso_ba_apply_res(ctx.h, wid))
            g2 = _readback(ctx, win, wid, True)
            for k in ("Je", "st", "act", "jp"):
                g[k] = g2[k]
            records = True
        else:
            records = path == "fused_records"
            ctx.check(ctx.L.sdso_ba_batch_create(ctx.h, 1, abi.ip(np.array([wid], np.int32))))
            ctx.check(ctx.L.sdso_ba_batch_set_materialize(ctx.h, int(records)))
            ctx.check(ctx.L.sdso_ba_batch_accumulate(ctx.h))
            g = _readback(ctx, win, wid, records)
        _compare(o, g, win["nr"], records)
    finally:
        ctx.check(ctx.L.sdso_ba_release_window(ctx.h, wid))


def test_batch_of_eleven_windows(gpu_ctx, batch_cases):
    ctx = gpu_ctx
    ids = np.array([100 + k for k in range(NBATCH)], np.int32)
    keeps = [_upload(ctx, case, int(ids[k]), 1000 + 10 * k) for k, case in enumerate(batch_cases)]
    try:
        ctx.check(ctx.L.sdso_ba_batch_create(ctx.h, NBATCH, abi.ip(ids)))
        ctx.check(ctx.L.sdso_ba_batch_set_materialize(ctx.h, 1))
        ctx.check(ctx.L.sdso_ba_batch_accumulate(ctx.h))
        assert len(set(case["win"]["nr"] for case in batch_cases)) > 1                # the windows differ: chunk counts are ragged
        for k, case in enumerate(batch_cases):
            g = _readback(ctx, case["win"], int(ids[k]), True)
            _compare(case["o"], g, case["win"]["nr"], True)
    finally:
        for k in ids:
            ctx.check(ctx.L.sdso_ba_release_window(ctx.h, int(k)))
    assert len(keeps) == NBATCH
