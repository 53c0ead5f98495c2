"""What stands between Python and a loaded libsdso_hip.so: the error type and the handle classes (sdso_shared, sdso_pool, sdso_ctx).

Context() raises if no MI355X/HIP device is usable: there is no CPU fallback."""
import ctypes as C

import numpy as np

from .abi_types import (c_float_p, PoolStats, InitPnts, InitPoints, TracePoints, ImmMatchOut, ImmActivate, ImmActivated, MapUpdate, MapCloud,
                        INIT_NCOUNTS, IMM_MATCH_NCOUNTS, IMM_ACT_NCOUNTS, MAP_REC_FLOATS)
from .abi_marshal import fp, ip, bp, bind, as_members, make_trace_points, make_distmap_geoms, make_flag_points
from .abi_lib import load


class SdsoError(RuntimeError):
    pass


class Shared:
    """One reference to an exported block of level buffers (sdso_shared); release() drops it."""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def info(self):
        """-> (kind: 0 pyramid / 1 template, device, holders: slots + handles)"""
        k, d, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        if self.L.sdso_shared_info(self.h, C.byref(k), C.byref(d), C.byref(n)) != 0:
            raise SdsoError("sdso_shared_info on a released handle")
        return k.value, d.value, n.value

    def release(self):
        if self.h:
            self.L.sdso_shared_release(self.h)
            self.h = None


class Pool:
    """The caller's reference to a device buffer pool (sdso_pool); release() drops it.  Attach ctxs with Context.set_pool."""

    def __init__(self, device=0, max_parked_bytes=1 << 30):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.sdso_pool_create(device, max_parked_bytes, C.byref(h))
        if rc != 0:
            raise SdsoError("sdso_pool_create(%d) failed with %d" % (device, rc))
        self.h = h

    def stats(self):
        """sdso_pool_stats -> dict of the counters"""
        st = PoolStats()
        if self.L.sdso_pool_stats(self.h, C.byref(st)) != 0:
            raise SdsoError("sdso_pool_stats on a released pool")
        return {k: getattr(st, k) for k, _ in PoolStats._fields_}

    def trim(self, keep_bytes=0):
        if self.L.sdso_pool_trim(self.h, keep_bytes) != 0:
            raise SdsoError("sdso_pool_trim on a released pool")

    def release(self):
        if self.h:
            self.L.sdso_pool_release(self.h)
            self.h = None


class Context:
    """One GPU + one HIP stream (sdso_ctx)."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.sdso_ctx_create(device, C.byref(h))
        if rc != 0:
            raise SdsoError("sdso_ctx_create(%d) failed with %d: no usable HIP device (no CPU fallback)" % (device, rc))
        self.h = h

    def check(self, rc):
        if rc != 0:
            msg = self.L.sdso_last_error(self.h)
            raise SdsoError("sdso call failed (%d): %s" % (rc, msg.decode() if msg else ""))

    def close(self):
        if self.h:
            self.L.sdso_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self.check(self.L.sdso_ctx_sync(self.h))

    def prof_read(self, kernel):
        ms = C.c_double(0)
        n = C.c_long(0)
        self.check(self.L.sdso_prof_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def ingest_frame(self, calib, slots, raws, exposure, factor=1.0):
        """sdso_ingest_frame for 1 or 2 raw images (uint8 / uint16 arrays); enqueue-only.  Returns exposure_out."""
        n = len(slots)
        arrs = [np.ascontiguousarray(r) for r in raws]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        ex = np.ascontiguousarray(exposure, np.float32)
        out = np.zeros(n, np.float32)
        self.check(self.L.sdso_ingest_frame(self.h, calib, n, (C.c_int * n)(*slots), ptrs, fp(ex), factor, fp(out)))
        return out

    def init_set_first_stereo(self, frame_slot, right_slot, K4, baseline, selection_map=None, read=True):
        """sdso_init_set_first_stereo -> (numPoints[0], counts); read=False: the enqueue-only form -> (None, None)."""
        K = np.ascontiguousarray(K4, np.float32)
        m = None if selection_map is None else np.ascontiguousarray(selection_map, np.float32)
        n = C.c_int(-1)
        counts = np.full(INIT_NCOUNTS, -1, np.int32)
        self.check(self.L.sdso_init_set_first_stereo(self.h, frame_slot, right_slot, fp(K), baseline, None if m is None else fp(m),
                                                     C.byref(n) if read else None, ip(counts) if read else None))
        return (n.value, counts) if read else (None, None)

    def init_get_pnts(self, cap):
        """sdso_init_get_pnts into arrays of cap entries -> dict of the Pnt members, cut to the n the library set."""
        d = dict(u=np.full(cap, -1, np.float32), v=np.full(cap, -1, np.float32), idepth=np.full(cap, -1, np.float32), iR=np.full(cap, -1, np.float32),
                 my_type=np.full(cap, -1, np.float32), status=np.full(cap, 254, np.uint8))
        P = bind(InitPnts(), d)
        P.n = -1
        self.check(self.L.sdso_init_get_pnts(self.h, C.byref(P)))
        assert 0 <= P.n <= cap
        return {k: a[:P.n] for k, a in d.items()}

    def init_from_initializer(self, keep=None, read=True):
        """sdso_init_from_initializer -> (points made, counts); read=False: the enqueue-only form -> (None, None)."""
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        n = C.c_int(-1)
        counts = np.full(4, -1, np.int32)
        self.check(self.L.sdso_init_from_initializer(self.h, None if k is None else bp(k), C.byref(n) if read else None, ip(counts) if read else None))
        return (n.value, counts) if read else (None, None)

    def init_get_points(self, cap):
        """sdso_init_get_points into arrays of cap entries -> dict of the PointHessian records, cut to the n the library set."""
        d = dict(pnt=np.full(cap, -1, np.int32))
        d.update({k: np.full(cap, -1, np.float32) for k in ("u", "v", "my_type", "idepth", "idepth_min", "idepth_max", "energyTH")})
        d.update(color=np.full((cap, 8), -1, np.float32), weights=np.full((cap, 8), -1, np.float32))
        P = bind(InitPoints(), d)
        P.n = -1
        self.check(self.L.sdso_init_get_points(self.h, C.byref(P)))
        assert 0 <= P.n <= cap
        return {k: a[:P.n] for k, a in d.items()}

    def imm_get(self, host_id):
        """sdso_imm_get: one host's immature points as a dict of numpy arrays (the members of ImmaturePoint, in the set's order)."""
        n = C.c_int(0)
        self.check(self.L.sdso_imm_count(self.h, host_id, C.byref(n)))
        n = n.value
        P, d = make_trace_points(n, np.zeros(n), np.zeros(n), np.zeros((n, 8)), np.zeros((n, 8)), np.zeros((n, 4)), np.zeros(n))
        P.idepth_min = None; P.idepth_stereo = None
        my_type = np.zeros(n, np.float32)
        self.check(self.L.sdso_imm_get(self.h, host_id, C.byref(P), fp(my_type)))
        assert P.n == n
        return dict(u=d["u_stereo"], v=d["v_stereo"], my_type=my_type, idepth_min=d["idepth_min_stereo"], idepth_max=d["idepth_max_stereo"],
                    quality=d["quality"], color=d["color"], weights=d["weights"], gradH=d["gradH"], energyTH=d["energyTH"],
                    lastTraceStatus=d["lastTraceStatus"], lastTraceUV=d["lastTraceUV"], lastTracePixelInterval=d["lastTracePixelInterval"])

    def imm_put(self, host_id, S, w, h):
        """sdso_imm_put_host: installs a group from a dict of arrays as imm_get returns it."""
        P = TracePoints()
        P.n = len(S["u"])
        d = {k: S[k] for k in ("color", "weights", "gradH", "energyTH", "quality", "lastTraceStatus", "lastTraceUV", "lastTracePixelInterval")}
        d.update(u_stereo=S["u"], v_stereo=S["v"], idepth_min_stereo=S["idepth_min"], idepth_max_stereo=S["idepth_max"])
        bind(P, as_members(P, d))
        my_type = np.ascontiguousarray(S["my_type"], np.float32)
        self.check(self.L.sdso_imm_put_host(self.h, host_id, w, h, C.byref(P), fp(my_type)))

    def imm_match_arrays(self, n, w=0, h=0, statuses=True):
        """An ImmMatchOut over fresh arrays for n points (and a w x h map where w > 0) -> (struct, dict of the arrays, counts)."""
        d = dict(accepted=np.full(n, 255, np.uint8), idepth=np.full((n, 3), -1, np.float32))
        if statuses:
            d.update(status_fwd=np.full(n, 254, np.uint8), status_back=np.full(n, 254, np.uint8))
        if w > 0:
            d["map"] = np.full((h, w, 3), -1, np.float32)
        return bind(ImmMatchOut(), d), d, np.full(IMM_MATCH_NCOUNTS, -1, np.int32)

    def imm_stereo_match(self, host_id, frame_slot, right_slot, K4, baseline, max_depth=70.0, map_wh=None, statuses=True):
        """sdso_imm_stereo_match: stereoMatch's loop (FullSystem.cpp:581-613) on one group -> dict of arrays: accepted, idepth [n, 3],
        status_fwd, status_back, counts and, with map_wh = (w, h) of the group's image, map [h, w, 3]."""
        n = C.c_int(0)
        self.check(self.L.sdso_imm_count(self.h, host_id, C.byref(n)))
        w, h = map_wh if map_wh else (0, 0)
        O, d, counts = self.imm_match_arrays(n.value, w, h, statuses)
        K = np.ascontiguousarray(K4, np.float32)
        self.check(self.L.sdso_imm_stereo_match(self.h, host_id, frame_slot, right_slot, fp(K), baseline, max_depth, 1 if map_wh else 0, C.byref(O), ip(counts)))
        d["counts"] = counts
        return d

    def imm_stereo_match_fetch(self, n, w=0, h=0, statuses=True):
        """sdso_imm_stereo_match_fetch -> the dict of imm_stereo_match for the latest call (n its group's count; a map where w > 0)."""
        O, d, counts = self.imm_match_arrays(n, w, h, statuses)
        self.check(self.L.sdso_imm_stereo_match_fetch(self.h, C.byref(O), ip(counts)))
        d["counts"] = counts
        return d

    def imm_stereo_map_dev(self):
        """sdso_imm_stereo_map_dev -> (device pointer, w, h)"""
        p, w, h = C.c_void_p(), C.c_int(0), C.c_int(0)
        self.check(self.L.sdso_imm_stereo_map_dev(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def imm_activate_raw(self, host_id, frame_slot, host_flagged, KRKi, Kt, pair_R, pair_t, pair_aff, w, h, K4, min_obs, min_act_dist, min_trace_quality=3.0):
        """sdso_imm_activate without the fetch -> (return code, counts)."""
        G = make_distmap_geoms(KRKi, Kt)
        A = ImmActivate()
        bind(A, as_members(A, dict(host_id=host_id, frame_slot=frame_slot, host_flagged=host_flagged, pair_R=pair_R, pair_t=pair_t, pair_aff=pair_aff)))
        A.nf = len(host_id); A.geom = C.cast(G, C.c_void_p)
        A.w, A.h, A.minObs, A.currentMinActDist, A.minTraceQuality = w, h, min_obs, min_act_dist, min_trace_quality
        A.K[:] = [float(x) for x in K4]
        counts = np.full(IMM_ACT_NCOUNTS, -1, np.int32)
        rc = self.L.sdso_imm_activate(self.h, C.byref(A), ip(counts))
        return rc, counts

    def imm_activate_fetch(self, n_candidates, n_selected, nf):
        """sdso_imm_activate_fetch -> dict of arrays (one entry per selected candidate) with `decision` (one per candidate)."""
        n = n_selected
        d = dict(frame=np.zeros(n, np.int32), index=np.zeros(n, np.int32), status=np.zeros(n, np.int8), idepth=np.zeros(n, np.float32),
                 res_state=np.zeros((n, nf), np.uint8), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), my_type=np.zeros(n, np.float32),
                 idepth_min=np.zeros(n, np.float32), idepth_max=np.zeros(n, np.float32), energyTH=np.zeros(n, np.float32),
                 color=np.zeros((n, 8), np.float32), weights=np.zeros((n, 8), np.float32), lastTraceStatus=np.zeros(n, np.uint8))
        O = bind(ImmActivated(), d)
        dec = np.zeros(n_candidates, np.uint8)
        self.check(self.L.sdso_imm_activate_fetch(self.h, C.byref(O), bp(dec)))
        assert O.n == n and O.nf == nf
        d["decision"] = dec
        return d

    def imm_activate(self, host_id, *args, **kw):
        """sdso_imm_activate + sdso_imm_activate_fetch -> (counts, dict of the activated records)."""
        rc, counts = self.imm_activate_raw(host_id, *args, **kw)
        self.check(rc)
        return counts, self.imm_activate_fetch(int(counts[0]), int(counts[4]), len(host_id))

    def distmap_make_from_window(self, wid, w, h, KRKi, Kt, skip=None, count=True):
        """sdso_distmap_make_from_window -> (return code, n_seeds); count=False passes n_seeds = NULL (no synchronisation) -> (rc, None).
        KRKi = None passes a null geom."""
        G = None if KRKi is None else make_distmap_geoms(KRKi, Kt)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        n = C.c_int(-1)
        rc = self.L.sdso_distmap_make_from_window(self.h, wid, w, h, G, None if sk is None else bp(sk), C.byref(n) if count else None)
        return rc, (n.value if count else None)

    def window_update_activated(self, wid, E, act_frame, cap):
        """sdso_ba_window_update_activated with the BAWindowEdit E -> (return code, n_points, n_res, act_index); act_frame = None passes a
        null map; cap: entries act_index is sized for (counts[4] of the activation)."""
        af = None if act_frame is None else np.ascontiguousarray(act_frame, np.int32)
        n_pt, n_res = C.c_int(-1), C.c_int(-1)
        idx = np.full(max(1, cap), -1, np.int32)
        rc = self.L.sdso_ba_window_update_activated(self.h, wid, C.byref(E), None if af is None else ip(af), C.byref(n_pt), C.byref(n_res), ip(idx))
        return rc, n_pt.value, n_res.value, idx[:max(0, n_pt.value)]

    def flag_points(self, wid, nf, npts, frame_marg, last_gone=None, **settings):
        """sdso_ba_flag_points -> (decision [np], counts [6], host_counts [nf, 6])."""
        F, keep = make_flag_points(frame_marg, last_gone, **settings)
        dec, cnt, hc = np.full(npts, 255, np.uint8), np.full(6, -1, np.int32), np.full((nf, 6), -1, np.int32)
        self.check(self.L.sdso_ba_flag_points(self.h, wid, C.byref(F), bp(dec), ip(cnt), ip(hc)))
        return dec, cnt, hc

    def keep_depth_map(self, on=True):
        """sdso_track_keep_depth_map: templates built from now on keep their level-0 map."""
        self.check(self.L.sdso_track_keep_depth_map(self.h, 1 if on else 0))

    def depth_image_raw(self, ref_slot, frame_slot, w, h, prev=None, rgb=True, idepth=True):
        """sdso_track_depth_image without the check -> (return code, dict).  prev = (minID, maxID) stands for *minID_pt / *maxID_pt,
        None for two null pointers; dict: rgb [h, w, 3] uint8, idepth [h, w], counts [2], range (the two values after the call, or None)."""
        d = dict(counts=np.full(2, -1, np.int32))
        if rgb:
            d["rgb"] = np.full((h, w, 3), 77, np.uint8)
        if idepth:
            d["idepth"] = np.full((h, w), -7, np.float32)
        r = None if prev is None else np.array(prev, np.float32)
        rc = self.L.sdso_track_depth_image(self.h, ref_slot, frame_slot, None if r is None else fp(r[0:1]), None if r is None else fp(r[1:2]),
                                           bp(d["rgb"]) if rgb else None, fp(d["idepth"]) if idepth else None, ip(d["counts"]))
        d["range"] = None if r is None else (r[0], r[1])
        return rc, d

    def depth_image(self, ref_slot, frame_slot, w, h, prev=None, rgb=True, idepth=True):
        """sdso_track_depth_image (debugPlotIDepthMap / debugPlotIDepthMapFloat on the slot's kept map) -> the dict of depth_image_raw."""
        rc, d = self.depth_image_raw(ref_slot, frame_slot, w, h, prev, rgb, idepth)
        self.check(rc)
        return d

    def depth_image_dev(self, ref_slot):
        """sdso_track_depth_image_dev -> (rgb device pointer, idepth device pointer, w, h)"""
        a, b, w, h = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
        self.check(self.L.sdso_track_depth_image_dev(self.h, ref_slot, C.byref(a), C.byref(b), C.byref(w), C.byref(h)))
        return a.value, b.value, w.value, h.value

    def map_update_raw(self, wid, active, gone, gone_list):
        """sdso_map_update without the check -> return code.  active: window point indices or None (every point not in gone)."""
        U = MapUpdate()
        d = as_members(U, dict(active=active, gone=gone, gone_list=gone_list))
        bind(U, d)
        U.n_active = 0 if active is None else len(d["active"])
        U.n_gone = len(d["gone"])
        return self.L.sdso_map_update(self.h, wid, C.byref(U))

    def map_update(self, wid, active, gone, gone_list):
        self.check(self.map_update_raw(wid, active, gone, gone_list))

    def map_counts(self, frame_id):
        """sdso_map_counts -> [active, marginalised, out]"""
        c = np.full(3, -1, np.int32)
        self.check(self.L.sdso_map_counts(self.h, frame_id, ip(c)))
        return c

    def map_get(self, frame_id, lst):
        """sdso_map_get -> records [n, 16] of list 1 (active), 2 (marginalised) or 3 (out)"""
        n = int(self.map_counts(frame_id)[lst - 1])
        r = np.full((n, MAP_REC_FLOATS), -9, np.float32)
        self.check(self.L.sdso_map_get(self.h, frame_id, lst, fp(r)))
        return r

    def map_put(self, frame_id, lst, records):
        r = np.ascontiguousarray(records, np.float32).reshape(-1, MAP_REC_FLOATS)
        self.check(self.L.sdso_map_put(self.h, frame_id, lst, len(r), fp(r)))

    def map_cloud_raw(self, frame_ids, K4, scaledTH=0.001, absTH=0.001, minBS=0.1, mode=1, imm_host_id=None, camToWorld=None, cap=None, bound=None):
        """sdso_map_cloud without the check -> (return code, dict: xyz [cap, 3], rgb [cap, 3] (untouched past n), first, kept [n_frames, 4], n).
        cap defaults to the bound 8 x the sum of the list sizes."""
        nfr = len(frame_ids)
        fid = np.ascontiguousarray(frame_ids, np.int32)
        imm = None if imm_host_id is None else np.ascontiguousarray(imm_host_id, np.int32)
        if cap is None:
            cap = 0
            for k in range(nfr):
                cap += 8 * int(self.map_counts(int(fid[k])).sum())
                if imm is not None and imm[k] >= 0:
                    n = C.c_int(0)
                    self.check(self.L.sdso_imm_count(self.h, int(imm[k]), C.byref(n)))
                    cap += 8 * n.value
        Q = MapCloud()
        bind(Q, as_members(Q, dict(frameID=fid, imm_host_id=imm, camToWorld=camToWorld)))
        Q.n_frames = nfr
        Q.fx, Q.fy, Q.cx, Q.cy = [float(x) for x in K4]
        Q.scaledTH, Q.absTH, Q.minBS, Q.mode = scaledTH, absTH, minBS, mode
        Q.cap = cap
        d = dict(xyz=np.full((max(cap, 1), 3), -77, np.float32), rgb=np.full((max(cap, 1), 3), 77, np.uint8), first=np.full(nfr + 1, -1, np.int32),
                 kept=np.full((nfr, 4), -1, np.int32))
        rc = self.L.sdso_map_cloud(self.h, C.byref(Q), fp(d["xyz"]), bp(d["rgb"]), ip(d["first"]), ip(d["kept"]))
        d["n"] = int(d["first"][nfr])
        return rc, d

    def map_cloud(self, frame_ids, K4, **kw):
        """sdso_map_cloud -> the dict of map_cloud_raw"""
        rc, d = self.map_cloud_raw(frame_ids, K4, **kw)
        self.check(rc)
        return d

    def map_cloud_dev(self):
        """sdso_map_cloud_dev -> (xyz device pointer, rgb device pointer, n)"""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self.check(self.L.sdso_map_cloud_dev(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def read_device(self, ptr, nbytes):
        """nbytes at a device pointer of this context, after its stream has drained (hipMemcpy through the HIP runtime the library uses)"""
        self.sync()
        out = np.zeros(nbytes, np.uint8)
        rc = self.L.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2)   # hipMemcpyDeviceToHost
        if rc != 0:
            raise SdsoError("hipMemcpy from the device failed (%d)" % rc)
        return out

    def export_pyramid(self, frame_slot):
        """sdso_pyramid_export -> Shared (one more holder of the slot's level buffers)"""
        h = C.c_void_p()
        self.check(self.L.sdso_pyramid_export(self.h, frame_slot, C.byref(h)))
        return Shared(self.L, h)

    def import_pyramid(self, frame_slot, shared):
        self.check(self.L.sdso_pyramid_import(self.h, frame_slot, shared.h))

    def export_ref(self, ref_slot):
        """sdso_track_export_ref -> Shared"""
        h = C.c_void_p()
        self.check(self.L.sdso_track_export_ref(self.h, ref_slot, C.byref(h)))
        return Shared(self.L, h)

    def import_ref(self, ref_slot, shared):
        self.check(self.L.sdso_track_import_ref(self.h, ref_slot, shared.h))

    def set_pool(self, pool):
        """sdso_ctx_set_pool; None detaches"""
        self.check(self.L.sdso_ctx_set_pool(self.h, pool.h if pool is not None else None))

    def slot_buffers(self, kind, slot):
        """sdso_shared_debug_buffers -> (device addresses of the SDSO_PYR_LEVELS level buffers, is_view)"""
        a = (C.c_ulonglong * 6)()
        v = C.c_int(0)
        self.check(self.L.sdso_shared_debug_buffers(self.h, kind, slot, a, C.byref(v)))
        return list(a), bool(v.value)

    def upload_pyramid(self, slot, pyr):
        n = len(pyr)
        ws = (C.c_int * n)(*[p.shape[1] for p in pyr])
        hs = (C.c_int * n)(*[p.shape[0] for p in pyr])
        arrs = [np.ascontiguousarray(p, np.float32) for p in pyr]
        ptrs = (c_float_p * n)(*[fp(a) for a in arrs])
        self.check(self.L.sdso_upload_pyramid(self.h, slot, n, ws, hs, ptrs))

    def set_ref(self, ref_slot, pc):
        for lvl, p in enumerate(pc):
            u, v, i, c = [np.ascontiguousarray(p[k], np.float32) for k in ("u", "v", "idepth", "color")]
            self.check(self.L.sdso_track_set_ref(self.h, ref_slot, lvl, len(u), fp(u), fp(v), fp(i), fp(c)))
