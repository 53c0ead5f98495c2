"""The device buffer pool (sdso_pool_*, csrc/pool.h + pool.hip): with a pool attached, the level buffers of pyramids, their level-0
copies and template levels are parked when they leave a slot and handed out again behind stream waits, so that the hand-off of
tests/test_handoff_gpu.py makes no allocator call and no host wait in its steady state.  The pool computes nothing, so every comparison is
by bit pattern against the same chain run on two ctxs WITHOUT a pool: stale or early-reused memory would show.  The counters
(sdso_pool_stats) say what the allocator saw.

320 x 240 (three levels); raw pairs of ingest_cases, a synth stereo pair for the level-0 copies, a synth tracker problem for the templates."""
import ctypes as C

import numpy as np
import pytest

import helpers
import ingest_cases as Cs
from sdso_amd import abi
import synth
import tracking_ref_window_cases as TC

pytestmark = pytest.mark.gpu

W, H = 320, 240
LEVELS = 3
ERR_ARG = -1
PYR, TPL = 0, 1
SIZE = dict(wOrg=W, hOrg=H, w=W, h=H)
CALIB = 7
SLOTS_A, SLOTS_B = (520, 521), (43, 44)
ZERO = dict(hits=0, misses=0, frees=0, host_waits=0, overflow_waits=0, parked_buffers=0, parked_bytes=0)
BIG = 1 << 30


@pytest.fixture(scope="module")
def raws():
    """nine raw pairs that differ"""
    return [[Cs.raw_image(W, H, 8, 100 + 2 * i), Cs.raw_image(W, H, 8, 101 + 2 * i)] for i in range(9)]


class Pair:
    """two fresh ctxs of device 0, A with an ingest calibration, both attached to `pool` (None: no pool)"""

    def __init__(self, pool):
        self.A, self.B = abi.Context(0), abi.Context(0)
        if pool is not None:
            self.A.set_pool(pool); self.B.set_pool(pool)
        assert Cs.calib_create(self.A, CALIB, SIZE, None, 8, Cs.response(8), Cs.vignette_inv(W, H), 2) == 0, self.A.L.sdso_last_error(self.A.h)

    def hand(self, raw_pair, slots_a=SLOTS_A, slots_b=SLOTS_B):
        """A ingests -> sdso_pyramid_export -> B imports -> the handles are released; nothing synchronises"""
        self.A.ingest_frame(CALIB, slots_a, raw_pair, (0.01, 0.02))
        for sa, sb in zip(slots_a, slots_b):
            h = self.A.export_pyramid(sa)
            self.B.import_pyramid(sb, h)
            h.release()

    def close(self):
        self.A.close(); self.B.close()


def frames_chain(pool, raws, n, on_frame=None):
    """n frames through a Pair -> what B downloads of every frame (both images, every level)"""
    P = Pair(pool)
    out = []
    try:
        for i in range(n):
            P.hand(raws[i])
            out.append([Cs.download_pyramid(P.B, s, W, H) for s in SLOTS_B])
            if on_frame:
                on_frame(i, P)
    finally:
        P.close()
    return out


@pytest.fixture(scope="module")
def unpooled_frames(raws):
    got = frames_chain(None, raws, 8)
    assert all(len(f[0]) == LEVELS for f in got) and not Cs.same_bits(got[0][0], got[1][0]) and not Cs.same_bits(got[0][0], got[0][1])
    return got


def same_frames(a, b):
    return len(a) == len(b) and all(Cs.same_bits(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def test_entry_points_and_fresh_stats():
    L = abi.load()
    for name in ("sdso_pool_create", "sdso_ctx_set_pool", "sdso_pool_stats", "sdso_pool_trim", "sdso_pool_release"):
        assert hasattr(L, name), name
    p = abi.Pool(0, BIG)
    try:
        assert p.stats() == ZERO
        p.trim(0)
        assert p.stats() == ZERO
    finally:
        p.release()


def test_steady_state_and_content(raws, unpooled_frames):
    pool = abi.Pool(0, BIG)
    stats, addrs = [], []

    def on_frame(i, P):
        stats.append(pool.stats())
        addrs.append([a for s in SLOTS_A for a in P.A.slot_buffers(PYR, s)[0][:LEVELS]])

    try:
        got = frames_chain(pool, raws, 8, on_frame)
        for i, s in enumerate(stats):
            print("frame", i, s)
        for i in range(2, 8):   # from the third frame on: no allocation, the level buffers of a pair per frame come out of the pool
            assert stats[i]["misses"] == stats[1]["misses"] == 4 * LEVELS, (i, stats[i])
            assert stats[i]["hits"] - stats[i - 1]["hits"] == 2 * LEVELS, (i, stats[i])
            assert set(addrs[i]) <= set(a for prev in addrs[:i] for a in prev), i
        assert all(s["host_waits"] == 0 and s["overflow_waits"] == 0 and s["frees"] == 0 for s in stats)
        assert same_frames(got, unpooled_frames)
        end = pool.stats()   # both ctxs are gone: what they held is parked
        assert end["misses"] == end["frees"] + end["parked_buffers"] and end["host_waits"] == 0
    finally:
        pool.release()


def _trace(ctx, pr, left, right):
    n = len(pr["u"])
    c, w, g, e = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    ctx.check(ctx.L.sdso_immature_init_batch(ctx.h, left, n, abi.fp(pr["u"]), abi.fp(pr["v"]), abi.fp(c), abi.fp(w), abi.fp(g), abi.fp(e)))
    P, d = abi.make_trace_points(n, pr["u"], pr["v"], c, w, g, e)
    st = np.zeros(n, np.uint8)
    K = np.array(pr["K"], np.float32)
    ctx.check(ctx.L.sdso_trace_stereo_batch(ctx.h, right, abi.fp(K), float(pr["calib"]["baseline"]), 1, C.byref(P), abi.bp(st)))
    return [c, e, st] + [d[k] for k in ("idepth_min_stereo", "idepth_max_stereo", "idepth_stereo", "lastTraceUV")]


def _derived_chain(pool, problems):
    """per stereo pair: A uploads it, B imports it, traces on it (plane0 is built by B) and releases its slots, so that the next pair's
    plane0 comes out of what the last one parked"""
    A, B = abi.Context(0), abi.Context(0)
    out = []
    try:
        if pool is not None:
            A.set_pool(pool); B.set_pool(pool)
        for pr in problems:
            A.upload_pyramid(540, [np.ascontiguousarray(pr["pyr_l"][0])]); A.upload_pyramid(541, [np.ascontiguousarray(pr["pyr_r"][0])])
            for sa, sb in ((540, 49), (541, 50)):
                h = A.export_pyramid(sa)
                B.import_pyramid(sb, h)
                h.release()
            out.append(_trace(B, pr, 49, 50))
            for s in (49, 50):
                B.check(B.L.sdso_release_pyramid(B.h, s))
    finally:
        A.close(); B.close()
    return out


def test_derived_copies_content():
    problems = [synth.stereo_problem(w=W, h=H, npts=300, seed=4031 + i) for i in range(3)]
    want = _derived_chain(None, problems)
    assert (want[0][2] == 0).sum() > 50 and not np.array_equal(TC.bits(want[0][5]), TC.bits(want[1][5]))
    pool = abi.Pool(0, BIG)
    try:
        got = _derived_chain(pool, problems)
        st = pool.stats()
        print(st)
        assert st["hits"] > 0 and st["host_waits"] == 0 and st["overflow_waits"] == 0
        for g_pair, w_pair in zip(got, want):
            for g, w in zip(g_pair, w_pair):
                assert np.array_equal(TC.bits(g), TC.bits(w))
    finally:
        pool.release()


def _eval_setup():
    cal = synth.kitti_calib(W, H)
    fx, fy, cx, cy = synth.level_intrinsics(cal["fx"], cal["fy"], cal["cx"], cal["cy"], LEVELS)
    prm = helpers.track_params(dict(levels=LEVELS, pyr_ref=[np.zeros((H >> l, W >> l, 3), np.float32) for l in range(LEVELS)], fx=fx, fy=fy, cx=cx, cy=cy))
    rs = np.random.RandomState(77)
    pc = []
    for l in range(LEVELS):
        wl, hl, n = W >> l, H >> l, 700 >> l
        pc.append(dict(u=rs.uniform(6, wl - 7, n).astype(np.float32), v=rs.uniform(6, hl - 7, n).astype(np.float32),
                       idepth=rs.uniform(0.05, 0.6, n).astype(np.float32), color=rs.uniform(20, 230, n).astype(np.float32)))
    nprob = 4
    evs = (abi.TrackEval * nprob)()
    for i in range(nprob):
        T = abi.SE3.from_Rt(*synth.se3_exp(rs.normal(0, 0.01, 6)))
        abi.load().sdso_track_make_eval(C.byref(prm), i % 2, C.byref(T), C.byref(abi.Aff(0.01, 0.5)), 1.0, C.byref(evs[i]))
    return pc, evs, nprob


def _in_flight(pool, raws, sync_before_drop):
    pc, evs, nprob = _eval_setup()
    P = Pair(pool)
    try:
        P.B.set_ref(1, pc)
        P.hand(raws[0])
        first = [a for s in SLOTS_A for a in P.A.slot_buffers(PYR, s)[0][:LEVELS]]
        P.A.ingest_frame(CALIB, SLOTS_A, raws[1], (0.01, 0.02))          # A's slots detach: B's slots are the last holders of frame 0
        refs, frames = (C.c_int * nprob)(*([1] * nprob)), (C.c_int * nprob)(*[SLOTS_B[i // 2] for i in range(nprob)])
        P.B.check(P.B.L.sdso_track_batch_prepare(P.B.h, nprob, refs, frames, evs))
        for _ in range(3):
            P.B.check(P.B.L.sdso_track_batch_enqueue(P.B.h))             # enqueue only
        if sync_before_drop:
            P.B.sync()
        for s in SLOTS_B:
            P.B.check(P.B.L.sdso_release_pyramid(P.B.h, s))              # the last holder leaves with work in flight
        P.A.ingest_frame(CALIB, (522, 523), raws[2], (0.01, 0.02))       # ... and A builds the next frame at once
        recycled = [a for s in (522, 523) for a in P.A.slot_buffers(PYR, s)[0][:LEVELS]]
        Hm, b, res, nw = np.zeros(nprob * 64), np.zeros(nprob * 8), np.zeros(nprob * 6), np.zeros(nprob, np.int32)
        P.B.check(P.B.L.sdso_track_batch_fetch(P.B.h, abi.dp(Hm), abi.dp(b), abi.dp(res), abi.ip(nw)))
        new = [Cs.download_pyramid(P.A, s, W, H) for s in (522, 523)]
    finally:
        P.close()
    return dict(out=(Hm.tobytes(), b.tobytes(), res.tobytes(), nw.tobytes()), nw=nw, first=first, recycled=recycled, new=new)


def test_in_flight(raws, unpooled_frames):
    """B drops a frame as its last holder with evaluations enqueued on it, and A writes the next frame into the same memory at once:
    the order between the two streams is the pool's doing (one run; an ordering check, not a search for a fault)"""
    pool = abi.Pool(0, BIG)
    try:
        got = _in_flight(pool, raws, False)
        st = pool.stats()
        want = _in_flight(pool, raws, True)
    finally:
        pool.release()
    plain = _in_flight(None, raws, True)
    print(st, got["nw"])
    assert set(got["recycled"]) == set(got["first"])                  # frame 2 went into the very buffers B was still reading
    assert st["host_waits"] == 0 and st["overflow_waits"] == 0 and st["hits"] == 2 * LEVELS
    assert (got["nw"] > 0).all()
    assert got["out"] == want["out"] == plain["out"]
    assert same_frames([got["new"]], [unpooled_frames[2]]) and same_frames([want["new"]], [unpooled_frames[2]])


@pytest.fixture(scope="module")
def tprob():
    return synth.tracker_problem(w=W, h=H, npts=1500, seed=7)


KF_POINTS = (600, 1500, 300, 1500)   # growing and shrinking
REF_A, REF_B, REF_OWN = 65, 31, 66


def _track(ctx, prm, ref, frame):
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    ctx.check(ctx.L.sdso_track_newest_coarse(ctx.h, ref, frame, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    R, t = T.Rt()
    return (np.asarray(R).tobytes(), np.asarray(t).tobytes(), aff.a, aff.b, out.good, out.evaluations, list(out.iterations),
            np.array(out.lastResiduals[:]).tobytes(), int(out.point_evals))


def _make_ref(ctx, ref_slot, frame_slot, tprob, n):
    u, v, idp = [np.ascontiguousarray(a[:n]) for a in tprob["points"]]
    pcn = np.zeros(8, np.int32)
    ctx.check(ctx.L.sdso_track_make_ref(ctx.h, ref_slot, frame_slot, n, abi.ip(u.astype(np.int32)), abi.ip(v.astype(np.int32)),
                                        abi.fp(idp.astype(np.float32)), abi.fp(np.ones(n, np.float32)), abi.ip(pcn)))
    return pcn


def _template_chain(pool, tprob):
    A, B = abi.Context(0), abi.Context(0)
    out = []
    try:
        if pool is not None:
            A.set_pool(pool); B.set_pool(pool)
        prm = helpers.track_params(tprob)
        A.upload_pyramid(600, tprob["pyr_ref"])
        B.upload_pyramid(51, tprob["pyr_new"])
        for n in KF_POINTS:
            _make_ref(A, REF_A, 600, tprob, n)
            h = A.export_ref(REF_A)
            B.import_ref(REF_B, h)
            h.release()
            _make_ref(A, REF_OWN, 600, tprob, n)   # a slot nobody exports: its levels grow in place (300 -> 1500)
            out.append(dict(levels=TC.get_ref(B, REF_B, LEVELS), own=TC.get_ref(A, REF_OWN, LEVELS), track=_track(B, prm, REF_B, 51),
                            stats=pool.stats() if pool is not None else None))
    finally:
        A.close(); B.close()
    return out


def _same_levels(a, b):
    return len(a) == len(b) and all(len(x["u"]) == len(y["u"]) and all(np.array_equal(TC.bits(x[k]), TC.bits(y[k])) for k in TC.KEYS) for x, y in zip(a, b))


def test_templates(tprob):
    want = _template_chain(None, tprob)
    assert len(want[1]["levels"][0]["u"]) > len(want[0]["levels"][0]["u"]) > len(want[2]["levels"][0]["u"]) > 100
    assert want[0]["track"][5] > 0 and want[0]["track"][8] > 0
    pool = abi.Pool(0, BIG)
    try:
        got = _template_chain(pool, tprob)
    finally:
        pool.release()
    for g in got:
        print(g["stats"])
    for g, w in zip(got, want):
        assert _same_levels(g["levels"], w["levels"]) and _same_levels(g["own"], w["own"])
        assert g["track"] == w["track"]
    end = got[-1]["stats"]
    assert end["hits"] > 0 and end["host_waits"] == 0 and end["overflow_waits"] == 0   # growth of REF_OWN's levels included


def test_cap(raws, unpooled_frames):
    """a pool that holds less than any level buffer parks nothing: every buffer goes today's way, behind a wait"""
    pool = abi.Pool(0, 4096)
    stats = []
    try:
        got = frames_chain(pool, raws, 4, lambda i, P: stats.append(pool.stats()))
        end = pool.stats()
    finally:
        pool.release()
    print(end)
    assert all(s["parked_buffers"] == 0 and s["parked_bytes"] == 0 and s["hits"] == 0 for s in stats + [end])
    assert end["overflow_waits"] > 0 and end["host_waits"] >= end["overflow_waits"] and end["frees"] == end["misses"]
    assert same_frames(got, unpooled_frames[:4])


def test_trim(raws):
    pool = abi.Pool(0, BIG)
    P = Pair(pool)
    try:
        for i in range(3):
            P.hand(raws[i])
        busy = pool.stats()
        pool.trim(0)                                               # work may still run on what is parked: only what has completed goes
        mid = pool.stats()
        assert mid["frees"] + mid["parked_buffers"] == busy["parked_buffers"] == 2 * LEVELS and mid["host_waits"] == 0
        for i in range(3, 6):                                      # (whatever the trim found, the chain goes on and a launch reports no error)
            P.hand(raws[i])
        assert Cs.same_bits(Cs.download_pyramid(P.B, SLOTS_B[0], W, H), Cs.download_pyramid(P.A, SLOTS_A[0], W, H))
        P.A.sync(); P.B.sync()
        before = pool.stats()
        pool.trim(0)
        after = pool.stats()
        print(before, after)
        assert before["parked_buffers"] == 2 * LEVELS and before["parked_bytes"] > 0
        assert after["parked_bytes"] == 0 and after["parked_buffers"] == 0 and after["frees"] - before["frees"] == before["parked_buffers"]
        assert after["host_waits"] == 0
        P.hand(raws[6])                                            # the chain goes on, on fresh memory
        assert Cs.download_pyramid(P.B, SLOTS_B[0], W, H)[0][0].any()
    finally:
        P.close(); pool.release()


def test_lifetime(raws, unpooled_frames):
    # the caller's reference outlives everything else: after the last handle every allocation is parked or freed
    pool = abi.Pool(0, BIG)
    P = Pair(pool)
    try:
        P.A.ingest_frame(CALIB, SLOTS_A, raws[0], (0.01, 0.02))
        h = P.A.export_pyramid(SLOTS_A[0])
        P.A.close()                                                # the ctx goes while its block lives on in the handle
        P.B.import_pyramid(SLOTS_B[0], h)
        assert Cs.same_bits(Cs.download_pyramid(P.B, SLOTS_B[0], W, H), unpooled_frames[0][0])
    finally:
        P.close()
    assert h.info() == (PYR, 0, 1)
    h.release()                                                    # no ctx: the block parks into its own pool
    st = pool.stats()
    print(st)
    assert st["misses"] == 2 * LEVELS and st["misses"] == st["frees"] + st["parked_buffers"] and st["host_waits"] == 0
    pool.release()
    # the caller's reference goes first, while ctxs and an unreleased handle refer to the pool; the handle goes last
    pool = abi.Pool(0, BIG)
    P = Pair(pool)
    try:
        P.hand(raws[1])
        h = P.A.export_pyramid(SLOTS_A[1])
        pool.release()
        P.hand(raws[2])                                            # the pool still serves its ctxs
        assert Cs.same_bits(Cs.download_pyramid(P.B, SLOTS_B[1], W, H), unpooled_frames[2][1])
    finally:
        P.close()
    assert h.info() == (PYR, 0, 1)
    h.release()


def test_refusals_and_isolation(raws, unpooled_frames):
    L = abi.load()
    out = C.c_void_p()
    st = abi.PoolStats()
    assert L.sdso_pool_create(0, 1, None) == ERR_ARG
    assert L.sdso_pool_create(-1, 1, C.byref(out)) != 0 and not out.value
    pool = abi.Pool(0, BIG)
    try:
        assert L.sdso_ctx_set_pool(None, pool.h) == ERR_ARG
        assert L.sdso_pool_stats(None, C.byref(st)) == ERR_ARG and L.sdso_pool_stats(pool.h, None) == ERR_ARG
        assert L.sdso_pool_trim(None, 0) == ERR_ARG
        L.sdso_pool_release(None)
        import torch
        if torch.cuda.device_count() > 1:
            other = abi.Pool(1, BIG)
            D = abi.Context(0)
            try:
                assert L.sdso_ctx_set_pool(D.h, other.h) == ERR_ARG and L.sdso_last_error(D.h)
            finally:
                D.close(); other.release()
        # a ctx without a pool leaves a bystander pool alone
        assert same_frames(frames_chain(None, raws, 2), unpooled_frames[:2])
        assert pool.stats() == ZERO
        # detaching returns a ctx to what it did before: its next release synchronises, and nothing reaches the pool
        P = Pair(pool)
        try:
            P.hand(raws[0])
            P.A.set_pool(None); P.B.set_pool(None)
            P.hand(raws[1]); P.hand(raws[2])                               # (the blocks made under the pool leave for it: their own pool)
            before = pool.stats()
            P.A.ingest_frame(CALIB, (524, 525), raws[3], (0.01, 0.02))     # enqueue only
            P.A.check(L.sdso_release_pyramid(P.A.h, 524))
            L.hipStreamQuery.argtypes = [C.c_void_p]
            L.sdso_ctx_stream.restype = C.c_void_p
            assert L.hipStreamQuery(L.sdso_ctx_stream(P.A.h)) == 0         # hipSuccess: the stream has drained
            P.hand(raws[4])
            assert Cs.same_bits(Cs.download_pyramid(P.B, SLOTS_B[0], W, H), Cs.download_pyramid(P.A, SLOTS_A[0], W, H))
            assert pool.stats() == before
            P.A.set_pool(pool); P.B.set_pool(pool)                         # ... and back again, any time
            P.hand(raws[5]); P.hand(raws[6])
            after = pool.stats()
            assert after["host_waits"] == 0 and after["hits"] + after["misses"] >= before["hits"] + before["misses"] + 4 * LEVELS   # the pool serves them again
        finally:
            P.close()
    finally:
        pool.release()
