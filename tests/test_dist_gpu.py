"""Sharded BA on the GPU: two processes share cuda:0, each owns half of the points of one window,
accumulates with libsdso_hip.so, the packed accumulators are summed with ONE collective (gloo here,
because two ranks cannot open RCCL on one device; bench.py --gpus N uses backend nccl == RCCL on
the same buffer), then both ranks stitch + solve and must obtain the x of the unsharded window."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _solve(ctx, abi, win, wid, slot0, reduce_fn=None):
    for f in range(win["nf"]):
        ctx.upload_pyramid(slot0 + f, win["pyrs"][f][:1])
    W, keep = abi.make_ba_window(win, frame_slots=[slot0 + f for f in range(win["nf"])])
    ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid, C.byref(W)))
    ctx.check(ctx.L.sdso_ba_linearize(ctx.h, wid, None))
    ctx.check(ctx.L.sdso_ba_apply_res(ctx.h, wid))
    ctx.check(ctx.L.sdso_ba_accumulate(ctx.h, wid))
    if reduce_fn is not None:
        acc = np.zeros(abi.accum_floats(win["nf"]), np.float32)
        ctx.check(ctx.L.sdso_ba_get_accumulators(ctx.h, wid, abi.fp(acc)))
        acc = reduce_fn(acc)
        ctx.check(ctx.L.sdso_ba_set_accumulators(ctx.h, wid, abi.fp(np.ascontiguousarray(acc))))
    n = 8 * win["nf"] + 4
    x, H = np.zeros(n), np.zeros((n, n))
    ctx.check(ctx.L.sdso_ba_solve(ctx.h, wid, 0, 0.1, abi.dp(x), abi.dp(H), None, None, None))
    step = np.zeros(win["np"], np.float32)
    ctx.check(ctx.L.sdso_ba_get_point_steps(ctx.h, wid, abi.fp(step)))
    return x, H, step


def _worker(rank, world, port, outdir):
    import torch.distributed as dist
    sys.path[:0] = [os.path.join(ROOT, "stereo-dso-g2o_amd")]
    from sdso_amd import abi, dist as sdist
    import synth
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = abi.Context(0)
    win = synth.ba_window(w=640, h=480, nf=5, pts_per_kf=100, seed=3031)
    sub, pidx, _ = sdist.shard_window(win, rank, world)
    x, H, step = _solve(ctx, abi, sub, 1, 10, reduce_fn=lambda a: sdist.allreduce_accumulators(a).numpy())
    np.save(os.path.join(outdir, "pidx_%d.npy" % rank), pidx)
    np.save(os.path.join(outdir, "x_%d.npy" % rank), x)
    np.save(os.path.join(outdir, "step_%d.npy" % rank), step)
    ctx.close()
    dist.destroy_process_group()


def test_two_rank_sharded_solve_matches_single(gpu_ctx, tmp_path):
    from sdso_amd import abi, dist as sdist
    import synth
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    win = synth.ba_window(w=640, h=480, nf=5, pts_per_kf=100, seed=3031)
    x, H, step = _solve(gpu_ctx, abi, win, 31, 90)
    xs = [np.load(tmp_path / ("x_%d.npy" % r)) for r in range(world)]
    assert np.array_equal(xs[0], xs[1])                         # identical reduced input -> identical solve on every rank
    d = np.sqrt(np.abs(np.diag(H))) + 1e-30
    assert np.abs((xs[0] - x) * d).max() <= 2e-4 * max(1.0, np.abs(x * d).max())
    steps = np.zeros(win["np"], np.float32)                     # every rank's points back in allPoints order (dist.shard_points: per-host slices)
    for r in range(world):
        steps[np.load(tmp_path / ("pidx_%d.npy" % r))] = np.load(tmp_path / ("step_%d.npy" % r))
    # (the sharded sums associate differently: x moves within the bar above, and a point's step is b - Hcd x carried through 1 / Hdd)
    assert np.abs(steps - step).max() <= 1e-3 * max(np.abs(step).max(), 1e-6)


@pytest.mark.gpu
def test_accumulator_block_is_aliased_by_torch(gpu_ctx):
    """bench.py all-reduces the packed accumulators IN PLACE through a torch tensor built on the library's device pointer
    (__cuda_array_interface__) on the ctx stream.  The tensor must alias the block, not copy it."""
    import torch
    from sdso_amd import abi
    import synth
    win = synth.ba_window(w=320, h=240, nf=4, pts_per_kf=40, seed=3091)
    nf = win["nf"]
    for f in range(nf):
        gpu_ctx.upload_pyramid(300 + f, win["pyrs"][f][:1])
    W, keep = abi.make_ba_window(win, frame_slots=[300 + f for f in range(nf)])
    gpu_ctx.check(gpu_ctx.L.sdso_ba_upload_window(gpu_ctx.h, 30, C.byref(W)))
    ids = np.array([30], np.int32)
    gpu_ctx.check(gpu_ctx.L.sdso_ba_batch_create(gpu_ctx.h, 1, abi.ip(ids)))
    gpu_ctx.check(gpu_ctx.L.sdso_ba_batch_accumulate(gpu_ctx.h))
    ptr, nfl = C.c_void_p(), C.c_long(0)
    gpu_ctx.check(gpu_ctx.L.sdso_ba_batch_accum_dev(gpu_ctx.h, C.byref(ptr), C.byref(nfl)))
    assert nfl.value == abi.accum_floats(nf)

    class Blob:
        __cuda_array_interface__ = {"shape": (nfl.value,), "typestr": "<f4", "data": (ptr.value, False), "version": 3}
    t = torch.as_tensor(Blob(), device="cuda")
    assert t.data_ptr() == ptr.value                                   # same memory
    stream = torch.cuda.ExternalStream(gpu_ctx.L.sdso_ctx_stream(gpu_ctx.h))
    before = np.zeros(nfl.value, np.float32)
    gpu_ctx.check(gpu_ctx.L.sdso_ba_get_accumulators(gpu_ctx.h, 30, abi.fp(before)))
    assert np.abs(before).max() > 0
    with torch.cuda.stream(stream):
        t.mul_(2.0)                                                    # stands in for the all-reduce of two equal shards
    after = np.zeros(nfl.value, np.float32)
    gpu_ctx.check(gpu_ctx.L.sdso_ba_get_accumulators(gpu_ctx.h, 30, abi.fp(after)))   # ctx stream: ordered after the torch op
    assert np.array_equal(after, 2.0 * before)


@pytest.mark.gpu
def test_library_allreduce_one_rank_is_identity():
    """The RCCL exchange inside the library (sdso_comm_* / sdso_ba_allreduce, csrc/comm.hip): a 1-rank communicator's sum is the
    identity, bit for bit, on the batch block and on one window's block; a second ctx of the process attaches to the same
    communicator; without a communicator the call is refused (SDSO_ERR_STATE), never silently skipped."""
    from sdso_amd import abi
    import synth
    ctx, ctx2 = abi.Context(0), abi.Context(0)
    try:
        L = ctx.L
        win = synth.ba_window(w=320, h=240, nf=4, pts_per_kf=40, seed=3093)
        nf = win["nf"]
        for c in (ctx, ctx2):
            for f in range(nf):
                c.upload_pyramid(320 + f, win["pyrs"][f][:1])
        W, keep = abi.make_ba_window(win, frame_slots=[320 + f for f in range(nf)])
        ids = np.array([33], np.int32)
        for c in (ctx, ctx2):
            c.check(L.sdso_ba_upload_window(c.h, 33, C.byref(W)))
            c.check(L.sdso_ba_batch_create(c.h, 1, abi.ip(ids)))
            c.check(L.sdso_ba_batch_accumulate(c.h))
        assert L.sdso_ba_allreduce(ctx.h) != 0                # no communicator yet: an error, not a no-op
        nr, rk = C.c_int(-5), C.c_int(-5)
        ctx.check(L.sdso_comm_info(ctx.h, C.byref(nr), C.byref(rk)))
        assert (nr.value, rk.value) == (0, -1)
        uid = (C.c_ubyte * 128)()
        assert L.sdso_comm_unique_id(uid) == 0
        assert any(uid)
        ctx.check(L.sdso_comm_init(ctx.h, 1, 0, uid))
        ctx2.check(L.sdso_comm_attach(ctx2.h, ctx.h))
        for c in (ctx, ctx2):
            c.check(L.sdso_comm_info(c.h, C.byref(nr), C.byref(rk)))
            assert (nr.value, rk.value) == (1, 0)
        n = 8 * nf + 4
        xs = []
        for c in (ctx, ctx2):
            before, after = np.zeros(abi.accum_floats(nf), np.float32), np.zeros(abi.accum_floats(nf), np.float32)
            c.check(L.sdso_ba_get_accumulators(c.h, 33, abi.fp(before)))
            assert np.abs(before).max() > 0
            c.check(L.sdso_ba_allreduce(c.h))
            c.check(L.sdso_ba_get_accumulators(c.h, 33, abi.fp(after)))
            assert np.array_equal(before, after)
            c.check(L.sdso_ba_batch_solve(c.h, 0.1, 0))
            x = np.zeros(n)
            c.check(L.sdso_ba_batch_get_x(c.h, abi.dp(x)))
            xs.append(x)
        assert np.array_equal(xs[0], xs[1]) and np.abs(xs[0]).max() > 0
        # the per-window form, between sdso_ba_accumulate and sdso_ba_solve (the shim's WindowedBA::allreduce)
        ctx.check(L.sdso_ba_upload_window(ctx.h, 34, C.byref(W)))
        ctx.check(L.sdso_ba_linearize(ctx.h, 34, None))
        ctx.check(L.sdso_ba_apply_res(ctx.h, 34))
        ctx.check(L.sdso_ba_accumulate(ctx.h, 34))
        before, after = np.zeros(abi.accum_floats(nf), np.float32), np.zeros(abi.accum_floats(nf), np.float32)
        ctx.check(L.sdso_ba_get_accumulators(ctx.h, 34, abi.fp(before)))
        assert np.abs(before).max() > 0
        ctx.check(L.sdso_ba_allreduce_window(ctx.h, 34))
        ctx.check(L.sdso_ba_get_accumulators(ctx.h, 34, abi.fp(after)))
        assert np.array_equal(before, after)
        # destroying the owner's handle keeps the communicator alive for the attached ctx
        ctx.check(L.sdso_comm_destroy(ctx.h))
        ctx2.check(L.sdso_ba_allreduce(ctx2.h))
        ctx2.check(L.sdso_comm_destroy(ctx2.h))
        assert L.sdso_ba_allreduce(ctx2.h) != 0
    finally:
        ctx2.close()
        ctx.close()


def _host_transport(dist, torch, world):
    """sdso_comm_init_host callbacks over torch.distributed (gloo) — two ranks cannot open RCCL on one device, and the library's
    collectives (all-reduce of the accumulators, all-gather of the resident loop's energy records) are transport-agnostic."""
    from sdso_amd import abi

    def allreduce(user, buf, n):
        t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(n,)))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return 0

    def allgather(user, send, recv, n):
        s = torch.from_numpy(np.ctypeslib.as_array(send, shape=(n,)).copy())
        out = [torch.empty(n, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(out, s)
        r = np.ctypeslib.as_array(recv, shape=(n * world,))
        for k, o in enumerate(out):
            r[k * n:(k + 1) * n] = o.numpy()
        return 0
    return abi.HOST_ALLREDUCE_FN(allreduce), abi.HOST_ALLGATHER_FN(allgather)


_OPT_SPECS = [dict(w=1232, h=368, nf=8, pts_per_kf=120, seed=3041), dict(w=640, h=480, nf=8, pts_per_kf=100, seed=3043, idepth_noise=0.3, state_noise=1e-2)]


def _batch_optimize(ctx, abi, wins, wid0, slot0, exchange_mode=0):
    nf = wins[0]["nf"]
    keep = []
    for k, win in enumerate(wins):
        for f in range(nf):
            ctx.upload_pyramid(slot0 + k * nf + f, win["pyrs"][f][:1])
        W, kp = abi.make_ba_window(win, frame_slots=[slot0 + k * nf + f for f in range(nf)])
        keep.append((W, kp))
        ctx.check(ctx.L.sdso_ba_upload_window(ctx.h, wid0 + k, C.byref(W)))
    ids = np.array([wid0 + k for k in range(len(wins))], np.int32)
    ctx.check(ctx.L.sdso_ba_batch_create(ctx.h, len(wins), abi.ip(ids)))
    ctx.check(ctx.L.sdso_ba_batch_exchange_mode(ctx.h, exchange_mode))
    res = (abi.BAOptResult * len(wins))()
    ctx.check(ctx.L.sdso_ba_batch_optimize(ctx.h, 6, res))
    out = []
    for k, win in enumerate(wins):
        s, i, r = np.zeros((nf, 10)), np.zeros(win["np"], np.float32), np.zeros(win["nr"], np.uint8)
        ctx.check(ctx.L.sdso_ba_get_state(ctx.h, wid0 + k, abi.dp(s), abi.fp(i), abi.bp(r)))
        out.append((s, i, r, res[k].iterations, res[k].resInA, res[k].lastEnergy))
    return out


_OPT_SPECS3 = _OPT_SPECS + [dict(w=640, h=480, nf=8, pts_per_kf=90, seed=3047)]


def _opt_worker(rank, world, port, outdir, gated=False, exchange_mode=0, tag="opt", specs=None, solver_bits=0):
    import torch
    import torch.distributed as dist
    sys.path[:0] = [os.path.join(ROOT, "stereo-dso-g2o_amd")]
    from sdso_amd import abi, dist as sdist
    import synth
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = abi.Context(0)
    cbs = _host_transport(dist, torch, world)
    ctx.check(ctx.L.sdso_comm_init_host(ctx.h, world, rank, cbs[0], cbs[1], None))
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import helpers
    shards = [sdist.shard_window(w, rank, world) for w in helpers.gen_windows(specs or _OPT_SPECS)]
    subs = [sh[0] for sh in shards]
    for k, sh in enumerate(shards):
        np.savez(os.path.join(outdir, "idx_%d_%d.npz" % (rank, k)), p=sh[1], r=sh[2])
    if gated:
        for w in subs:
            w["forceAcceptStep"] = 0
    for w in subs:
        w["solverMode"] = int(w["solverMode"]) | solver_bits
    out = _batch_optimize(ctx, abi, subs, 1, 10, exchange_mode)
    for k, (s, i, r, its, resInA, e) in enumerate(out):
        np.savez(os.path.join(outdir, "%s_%d_%d.npz" % (tag, rank, k)), s=s, i=i, r=r, its=its, resInA=resInA, e=e)
    ctx.close()
    dist.destroy_process_group()


def test_two_rank_sharded_gn_loop_matches_single(gpu_ctx, oracle, tmp_path):
    """The whole Gauss-Newton loop over sharded windows (sdso_ba_batch_optimize on 2 ranks: per iteration one all-reduce of the packed
    accumulators and one all-gather of the newest-frame energies / break-test sums) takes the decisions of the unsharded window on every
    rank: same iteration count, same quantile thresholds (through the residual states), states / idepths within 1e-5 + twice the
    oracle's own order-of-summation spread."""
    from sdso_amd import abi
    import synth
    import helpers
    world = 2
    mp.spawn(_opt_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    import helpers
    wins = helpers.gen_windows(_OPT_SPECS)
    single = _batch_optimize(gpu_ctx, abi, wins, 41, 600)
    for k, win in enumerate(wins):
        nf, npts, nr = win["nf"], win["np"], win["nr"]
        sh = [np.load(tmp_path / ("opt_%d_%d.npz" % (r, k))) for r in range(world)]
        s1, i1, r1, its1, resInA1, e1 = single[k]
        assert int(sh[0]["its"]) == int(sh[1]["its"]) == its1
        assert np.array_equal(sh[0]["s"], sh[1]["s"])                        # identical reduced systems -> identical states on every rank
        assert int(sh[0]["resInA"]) == int(sh[1]["resInA"])
        # order-of-summation spread of the CPU arithmetic on this window
        W, keep = abi.make_ba_window(win, frame_slots=list(range(nf)), dI_list=[p[0] for p in win["pyrs"]])
        h = oracle.orc_ba_create(C.byref(W))
        so, io, ro, oo = np.zeros((nf, 10)), np.zeros(npts, np.float32), np.zeros(nr, np.uint8), abi.BAOptResult()
        oracle.orc_ba_optimize(h, 6, abi.dp(so), abi.fp(io), abi.bp(ro), C.byref(oo))
        oracle.orc_ba_destroy(h)
        ss, si = 0.0, 0.0
        for seed in (1, 3):
            w2, order = helpers.permuted_window(win, seed)
            W2, keep2 = abi.make_ba_window(w2, frame_slots=list(range(nf)), dI_list=[p[0] for p in win["pyrs"]])
            h2 = oracle.orc_ba_create(C.byref(W2))
            sp, ip, rp, op = np.zeros((nf, 10)), np.zeros(npts, np.float32), np.zeros(nr, np.uint8), abi.BAOptResult()
            oracle.orc_ba_optimize(h2, 6, abi.dp(sp), abi.fp(ip), abi.bp(rp), C.byref(op))
            oracle.orc_ba_destroy(h2)
            ss, si = max(ss, np.abs(sp - so).max()), max(si, np.abs(ip - io[order]).max())
        idep, rst = np.zeros(npts, np.float32), np.zeros(nr, np.uint8)       # back in the global window's order
        for r in range(world):
            ix = np.load(tmp_path / ("idx_%d_%d.npz" % (r, k)))
            idep[ix["p"]] = sh[r]["i"]; rst[ix["r"]] = sh[r]["r"]
        assert np.abs(sh[0]["s"] - s1).max() <= 1e-5 + 2.0 * ss, (np.abs(sh[0]["s"] - s1).max(), ss)
        assert helpers.idepths_close(idep, i1, 1e-5 + 2.0 * si), (np.abs(idep - i1).max(), si)
        assert (rst != r1).sum() <= max(2, nr // 2000)
        assert helpers.counts_close(int(sh[0]["resInA"]), resInA1, nr)
        esum = float(sh[0]["e"])
        assert abs(esum - e1) <= 1e-4 * e1                                   # lastEnergy is the all-gathered sum on every rank
    for k in range(len(wins)):
        gpu_ctx.check(gpu_ctx.L.sdso_ba_release_window(gpu_ctx.h, 41 + k))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [512, 1024])
def test_two_rank_sharded_momentum_loops_match_single(gpu_ctx, tmp_path, bits):
    """SOLVER_MOMENTUM (512) / SOLVER_STEPMOMENTUM (1024) over sharded windows: every rank solves the all-reduced system, runs k_ba_opt_momentum on
    the same x (the stepsize, previousX and the kept steps are rank-local copies of the same values), steps its own points, and the frames'
    step goes through the all-gathered break-test sums — the ranks end on identical states, equal to the unsharded batch's up to the float
    addition of the two ranks' packed blocks.  (Such windows never take the reduce-scatter exchange: asked for here, refused by agreement.)"""
    from sdso_amd import abi
    import helpers
    world = 2
    mp.spawn(_opt_worker, args=(world, _free_port(), str(tmp_path), False, 1, "mom", None, bits), nprocs=world, join=True)
    wins = [dict(w) for w in helpers.gen_windows(_OPT_SPECS)]
    for w in wins:
        w["solverMode"] = int(w["solverMode"]) | bits
    single = _batch_optimize(gpu_ctx, abi, wins, 41, 600)
    for k, win in enumerate(wins):
        npts, nr = win["np"], win["nr"]
        sh = [np.load(tmp_path / ("mom_%d_%d.npz" % (r, k))) for r in range(world)]
        s1, i1, r1, its1, resInA1, e1 = single[k]
        assert int(sh[0]["its"]) == int(sh[1]["its"]) == its1
        assert np.array_equal(sh[0]["s"], sh[1]["s"])
        idep, rst = np.zeros(npts, np.float32), np.zeros(nr, np.uint8)
        for r in range(world):
            ix = np.load(tmp_path / ("idx_%d_%d.npz" % (r, k)))
            idep[ix["p"]] = sh[r]["i"]; rst[ix["r"]] = sh[r]["r"]
        flips = int((rst != r1).sum())
        assert flips <= max(2, nr // 2000)
        # (the two ranks' packed blocks are floats added in float, the single GPU rounds its f64 sums once: 1e-7 relative on the accumulators, which the
        #  momentum modes feed from step to step — measured 2.4e-5 on the noisy window; a residual flipping on its threshold moves the following updates
        #  by more: tests/test_ba_solver_bits_gpu.py)
        bar = 5e-5 if flips == 0 else 2e-4
        assert np.abs(sh[0]["s"] - s1).max() <= bar, (np.abs(sh[0]["s"] - s1).max(), flips)
        assert helpers.idepths_close(idep, i1, 10 * bar)
        assert abs(float(sh[0]["e"]) - e1) <= 1e-4 * e1
    for k in range(len(wins)):
        gpu_ctx.check(gpu_ctx.L.sdso_ba_release_window(gpu_ctx.h, 41 + k))


@pytest.mark.gpu
def test_two_rank_sharded_energy_gated_loop_matches_single(gpu_ctx, tmp_path):
    """setting_forceAceptStep = false over sharded windows (FullSystemOptimize.cpp:961-990): besides the all-reduce of the accumulators and
    the all-gather of the break-test sums, every trial linearisation is followed by an all-gather of the ranks' newest-frame energies,
    residual energies and calcLEnergy parts, and the gate reads them rank by rank — so both ranks take the same accept / reject decisions
    (identical states on every rank) and they are the decisions of the unsharded window (same iteration count, states / idepths within the
    sharded accepted-step loop's bars)."""
    from sdso_amd import abi
    import synth
    import helpers
    world = 2
    mp.spawn(_opt_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    import helpers
    wins = helpers.gen_windows(_OPT_SPECS)
    for w in wins:
        w["forceAcceptStep"] = 0
    single = _batch_optimize(gpu_ctx, abi, wins, 51, 700)
    for k, win in enumerate(wins):
        npts, nr = win["np"], win["nr"]
        sh = [np.load(tmp_path / ("opt_%d_%d.npz" % (r, k))) for r in range(world)]
        s1, i1, r1, its1, resInA1, e1 = single[k]
        assert int(sh[0]["its"]) == int(sh[1]["its"]) == its1
        assert np.array_equal(sh[0]["s"], sh[1]["s"])                        # the same decisions and the same reduced systems on every rank
        assert int(sh[0]["resInA"]) == int(sh[1]["resInA"])
        idep, rst = np.zeros(npts, np.float32), np.zeros(nr, np.uint8)       # back in the global window's order
        for r in range(world):
            ix = np.load(tmp_path / ("idx_%d_%d.npz" % (r, k)))
            idep[ix["p"]] = sh[r]["i"]; rst[ix["r"]] = sh[r]["r"]
        assert np.abs(sh[0]["s"] - s1).max() <= 1e-4, np.abs(sh[0]["s"] - s1).max()
        assert helpers.idepths_close(idep, i1, 2e-4), np.abs(idep - i1).max()
        assert (rst != r1).sum() <= max(2, nr // 2000)
        assert abs(float(sh[0]["e"]) - e1) <= 1e-4 * e1
    for k in range(len(wins)):
        gpu_ctx.check(gpu_ctx.L.sdso_ba_release_window(gpu_ctx.h, 51 + k))


@pytest.mark.gpu
def test_three_ranks_three_windows_both_exchange_shapes(gpu_ctx, tmp_path):
    """The two shapes of the exchange on three ranks (every host keyframe's points cut three ways — a rank count that divides neither the
    keyframes nor a power of two).  Shape 1 (sdso_ba_batch_exchange_mode(ctx, 1), csrc/comm.hip reduce_scatter_block): the reduce-scatter
    leaves rank r with the summed accumulators of ITS window only (the other slices keep this rank's partial sums, as RCCL leaves
    them), the fused tail kernel solves that window, and x / xAd / nres travel to the other ranks by all-gather.  The sums are the same
    numbers and the solve is deterministic, so every rank must end on the bits of the all-reduce run — states, idepths, residual
    states, iteration counts — and those are the unsharded loop's decisions with states inside the sharded loop's bar."""
    from sdso_amd import abi
    import synth
    world = 3
    for mode, tag in ((0, "ar3"), (1, "rs3")):
        mp.spawn(_opt_worker, args=(world, _free_port(), str(tmp_path), False, mode, tag, _OPT_SPECS3), nprocs=world, join=True)
    import helpers
    wins = helpers.gen_windows(_OPT_SPECS3)
    single = _batch_optimize(gpu_ctx, abi, wins, 61, 800)
    for k in range(len(_OPT_SPECS3)):
        ref = np.load(tmp_path / ("ar3_0_%d.npz" % k))
        for r in range(world):
            a, b = np.load(tmp_path / ("ar3_%d_%d.npz" % (r, k))), np.load(tmp_path / ("rs3_%d_%d.npz" % (r, k)))
            assert int(a["its"]) == int(b["its"]) == int(ref["its"]) and int(a["resInA"]) == int(b["resInA"])
            assert np.array_equal(a["s"], b["s"]) and np.array_equal(a["i"], b["i"]) and np.array_equal(a["r"], b["r"])
            assert np.array_equal(a["s"], ref["s"])                           # every rank holds the same frame states
        assert int(ref["its"]) == single[k][3]
        assert np.abs(ref["s"] - single[k][0]).max() <= 1e-4, np.abs(ref["s"] - single[k][0]).max()
    for k in range(len(wins)):
        gpu_ctx.check(gpu_ctx.L.sdso_ba_release_window(gpu_ctx.h, 61 + k))


def _two_comm_worker(rank, world, port, outdir):
    """Two contexts per process, each with its OWN communicator (its own gloo group underneath), each running the sharded GN loop of its
    own batch on its own host thread at the same time — what a FullSystem with two mapping threads, or bench.py's two stream groups with
    one communicator each, would do.  Nothing orders the collectives of the two communicators against each other."""
    import threading
    import torch
    import torch.distributed as dist
    sys.path[:0] = [os.path.join(ROOT, "stereo-dso-g2o_amd"), os.path.join(ROOT, "tests")]
    from sdso_amd import abi, dist as sdist
    import synth
    import helpers
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    groups = [dist.new_group(list(range(world)), backend="gloo") for _ in range(2)]
    ctxs, cbs, subs = [], [], []
    for g in range(2):
        ctx = abi.Context(0)

        class _G:                      # the callbacks of communicator g talk to group g only
            @staticmethod
            def all_reduce(t, op, grp=groups[g]): return dist.all_reduce(t, op=op, group=grp)
            @staticmethod
            def all_gather(out, s, grp=groups[g]): return dist.all_gather(out, s, group=grp)
            ReduceOp = dist.ReduceOp
        cb = _host_transport(_G, torch, world)
        ctx.check(ctx.L.sdso_comm_init_host(ctx.h, world, rank, cb[0], cb[1], None))
        ctxs.append(ctx); cbs.append(cb)
        # both batches hold both windows, in opposite order: the same work, different collectives in flight at any one time
        specs = _OPT_SPECS if g == 0 else _OPT_SPECS[::-1]
        subs.append([sdist.shard_window(w, rank, world)[0] for w in helpers.gen_windows(specs)])
    outs, errs = [None, None], []

    def run(g):
        try:
            outs[g] = _batch_optimize(ctxs[g], abi, subs[g], 1, 10, exchange_mode=g)     # (and one communicator of each exchange shape)
        except BaseException as e:     # noqa: BLE001 — reported by the parent through the missing file
            errs.append(repr(e))
    th = [threading.Thread(target=run, args=(g,)) for g in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    assert not errs, errs
    for g in range(2):
        order = [0, 1] if g == 0 else [1, 0]
        for j, (s, i, r, its, resInA, e) in enumerate(outs[g]):
            np.savez(os.path.join(outdir, "tc%d_%d_%d.npz" % (g, rank, order[j])), s=s, i=i, r=r, its=its, resInA=resInA, e=e)
    for ctx in ctxs:
        ctx.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_communicators_per_process_on_separate_threads(tmp_path):
    """Round-3 verdict, multi-GPU readiness (d): two communicators per process over the host transport, driven from two host threads at
    once.  Each must reproduce the run of one communicator alone, bit for bit — any sharing of staging buffers, registry entries or
    stream state between the two contexts would show as a difference (or a deadlock: the test runs under the suite's timeout)."""
    world = 2
    mp.spawn(_opt_worker, args=(world, _free_port(), str(tmp_path), False, 0, "ref"), nprocs=world, join=True)
    mp.spawn(_two_comm_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for k in range(len(_OPT_SPECS)):
        for r in range(world):
            ref = np.load(tmp_path / ("ref_%d_%d.npz" % (r, k)))
            for g in range(2):
                got = np.load(tmp_path / ("tc%d_%d_%d.npz" % (g, r, k)))
                assert int(got["its"]) == int(ref["its"]) and int(got["resInA"]) == int(ref["resInA"]), (g, r, k)
                assert np.array_equal(got["s"], ref["s"]) and np.array_equal(got["i"], ref["i"]) and np.array_equal(got["r"], ref["r"]), (g, r, k)


@pytest.mark.gpu
def test_resident_loop_through_rccl_one_rank(monkeypatch):
    """The RCCL collectives of the resident loop on the one GPU this box has: with a 1-rank communicator and SDSO_OPT_FORCE_EXCHANGE=1
    sdso_ba_batch_optimize takes the multi-rank path — ncclAllReduce(max) of the pack capacity, per iteration ncclAllReduce of the
    accumulators, k_ba_opt_pack and ncclAllGather of the energy records — and must reproduce the plain single-rank run bit for bit."""
    from sdso_amd import abi
    import synth
    import helpers
    wins = helpers.gen_windows(_OPT_SPECS)
    outs = {}
    for mode in ("plain", "rccl", "rccl_scatter"):
        ctx = abi.Context(0)
        try:
            if mode != "plain":
                uid = (C.c_ubyte * 128)()
                assert ctx.L.sdso_comm_unique_id(uid) == 0
                ctx.check(ctx.L.sdso_comm_init(ctx.h, 1, 0, uid))
                monkeypatch.setenv("SDSO_OPT_FORCE_EXCHANGE", "1")
            else:
                monkeypatch.delenv("SDSO_OPT_FORCE_EXCHANGE", raising=False)
            outs[mode] = _batch_optimize(ctx, abi, wins, 1, 10, exchange_mode=1 if mode == "rccl_scatter" else 0)
        finally:
            monkeypatch.delenv("SDSO_OPT_FORCE_EXCHANGE", raising=False)
            ctx.close()
    # rccl_scatter: ncclReduceScatter in place + ncclAllGather in place of the solution records (1 rank: every window is this rank's)
    for other in ("rccl", "rccl_scatter"):
        for a, b in zip(outs["plain"], outs[other]):
            assert a[3] == b[3] and a[4] == b[4]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert a[5] == b[5]


# ------------------------------------------------------------------ `bench.py --gpus 2` itself, as a command
@pytest.mark.parametrize("scaling", ["weak", "strong", "weak_scatter"])
def test_bench_command_two_ranks_advances_the_same_work(scaling):
    """`python3 bench.py --gpus 2` with NO launcher around it: main() must start its two ranks itself (round-4 verdict: the flag was
    parsed and ignored, so the first real scaling run would have measured one GPU) and print ONE line that says n_gpus 2.  The step
    is the full one (state_advances), window 0's sharded x equals the unsharded window's, the GN steps shrink.  Two ranks cannot
    open RCCL on the one device of the test box: SDSO_DIST_BACKEND=gloo_lib runs the library's exchange over its host transport.
    weak_scatter: SDSO_BA_EXCHANGE=scatter (reduce-scatter by window + all-gather of x inside the timed step)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["SDSO_DIST_BACKEND"] = "gloo_lib"
    env["SDSO_BA_EXCHANGE"] = "scatter" if scaling.endswith("_scatter") else "allreduce"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "3", "--batch", "4", "--full",
           "--scaling", scaling.replace("_scatter", "")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3
    assert out["scaling"] == scaling.replace("_scatter", "")
    cfg, extra = out["config"], out["extra"]
    assert cfg["state_advances"] is True and cfg["allreduce_floats"] > 0
    assert ("reduce-scatter" in cfg["exchange_shape"]) == scaling.endswith("_scatter")
    assert "host transport" in cfg["exchange"]
    assert extra["sharded_x_whitened_err"] <= 2e-4
    assert extra["max_abs_x"] < extra["max_abs_x_initial"]
    assert out["roofline"]["launches"] > 0 and out["value"] > 0
    # what the first real scaling run has to prove by itself (round-5 verdict, item 6): the communicator the LIBRARY holds has two ranks
    # (sdso_comm_info, not WORLD_SIZE), and the exchange is in the line with its bytes, its calls and its HIP-event time per step
    assert cfg["rccl_ranks"] == 2 and cfg["launcher_world_size"] == 2
    assert extra["exchange_bytes_per_step"] == 4 * cfg["allreduce_floats"] > 0
    assert extra["exchange_ms_per_step"] > 0 and extra["exchange_calls_per_step"] >= 1
