"""Inputs for the distance-map / candidate-selection tests and thin ctypes wrappers of the four entry points."""
import ctypes as C

import numpy as np

import synth

f32 = np.float32


def window_geoms(evalPT, K, levels=2):
    """KRKi = K[1] * R * Ki[0], Kt = K[1] * t of every keyframe but the newest into the newest, as CoarseTracker.cpp:1232-1236 forms them
    (the float products are the caller's side of the interface: any float values do for a parity test)."""
    fxs, fys, cxs, cys = synth.level_intrinsics(*K, levels)
    K1 = np.array([[fxs[1], 0, cxs[1]], [0, fys[1], cys[1]], [0, 0, 1]], f32)
    K0 = np.array([[fxs[0], 0, cxs[0]], [0, fys[0], cys[0]], [0, 0, 1]], np.float64)
    Ki0 = np.linalg.inv(K0).astype(f32)
    nf = len(evalPT)
    T = [(np.asarray(e[:9], np.float64).reshape(3, 3), np.asarray(e[9:], np.float64)) for e in evalPT]
    KRKi, Kt = [], []
    for g in range(nf - 1):
        R, t = synth.se3_mul(T[nf - 1], synth.se3_inv(T[g]))
        KRKi.append((K1 @ R.astype(f32)) @ Ki0)
        Kt.append(K1 @ t.astype(f32))
    return np.array(KRKi, f32), np.array(Kt, f32)


def forward_geoms(w, h, nhost, seed):
    """nhost keyframes behind the newest one on a forward trajectory with a little rotation."""
    rs = np.random.RandomState(seed)
    cal = synth.kitti_calib(w, h)
    K = (cal["fx"], cal["fy"], cal["cx"], cal["cy"])
    ev = []
    for k in range(nhost + 1):
        xi = np.array([0, 0, -0.2 * k, 0, 0, 0], np.float64)
        xi[3:] = rs.normal(0, 0.01, 3)
        xi[0:2] = rs.normal(0, 0.02, 2)
        ev.append(synth.se3_pack(synth.se3_exp(xi)))
    return window_geoms(np.array(ev), K)


def selection_case(w=1232, h=368, nhost=7, per_host=2000, n_active=2600, min_act_dist=2.0, seed=1):
    """Active points (the seeds of the map) and immature candidates of `nhost` keyframes, uniformly spread, with every gate of
    activatePointsMT STEP 2 firing for a few per cent of the candidates."""
    rs = np.random.RandomState(seed)
    KRKi, Kt = forward_geoms(w, h, nhost, seed + 17)
    a = dict(pg=np.sort(rs.randint(0, nhost, n_active)).astype(np.int32), u=rs.uniform(3, w - 4, n_active).astype(f32), v=rs.uniform(3, h - 4, n_active).astype(f32),
             idepth=rs.uniform(0.01, 0.15, n_active).astype(f32))
    n = nhost * per_host
    mid = rs.uniform(0.01, 0.15, n)
    rel = rs.uniform(0.02, 0.3, n)
    c = dict(pg=np.repeat(np.arange(nhost), per_host).astype(np.int32), u=rs.uniform(3, w - 4, n).astype(f32), v=rs.uniform(3, h - 4, n).astype(f32),
             idepth_min=(mid * (1 - rel)).astype(f32), idepth_max=(mid * (1 + rel)).astype(f32))
    # ImmaturePointStatus: GOOD 0, OOB 1, OUTLIER 2, SKIPPED 3, BADCONDITION 4, UNINITIALIZED 5
    c["status"] = rs.choice(6, n, p=[0.62, 0.04, 0.04, 0.14, 0.12, 0.04]).astype(np.uint8)
    c["idepth_max"][rs.rand(n) < 0.03] = np.nan                       # never traced successfully
    neg = rs.rand(n) < 0.02                                           # idepth_max + idepth_min <= 0
    c["idepth_min"][neg] = -np.abs(c["idepth_max"][neg]) - f32(0.01)
    c["quality"] = np.where(rs.rand(n) < 0.05, rs.uniform(1, 3, n), rs.uniform(3.01, 12, n)).astype(f32)
    c["quality"][rs.rand(n) < 0.01] = f32(3.0)                        # exactly on the bar: `>` fails
    c["interval"] = np.where(rs.rand(n) < 0.05, rs.uniform(8, 20, n), rs.uniform(0, 7.99, n)).astype(f32)
    c["my_type"] = rs.choice([1.0, 2.0, 4.0], n, p=[0.6, 0.25, 0.15]).astype(f32)
    flagged = np.zeros(nhost, np.uint8)
    flagged[0] = 1
    return dict(w=w, h=h, KRKi=KRKi, Kt=Kt, active=a, cand=c, flagged=flagged, min_act_dist=f32(min_act_dist), min_trace_quality=f32(3.0))


# the three regimes of the selection test: currentMinActDist with about 1 200 / 2 000 / 3 200 seeds
REGIMES = {"dense_0.7": dict(min_act_dist=0.7, n_active=1330, seed=11), "mid_2": dict(min_act_dist=2.0, n_active=2220, seed=12),
           "sparse_4": dict(min_act_dist=4.0, n_active=3550, seed=13)}


# ------------------------------------------------------------------ the C-ABI
def dm_make(ctx, w, h, KRKi, Kt, pg, u, v, idepth):
    from sdso_amd import abi
    G = abi.make_distmap_geoms(KRKi, Kt)
    pg, u, v, idepth = np.ascontiguousarray(pg, np.int32), np.ascontiguousarray(u, f32), np.ascontiguousarray(v, f32), np.ascontiguousarray(idepth, f32)
    ns = C.c_int(-1)
    ctx.check(ctx.L.sdso_distmap_make(ctx.h, w, h, len(np.asarray(KRKi).reshape(-1, 9)), G, len(u), abi.ip(pg), abi.fp(u), abi.fp(v), abi.fp(idepth), C.byref(ns)))
    return ns.value


def dm_get(ctx, w, h):
    from sdso_amd import abi
    m = np.full((h >> 1, w >> 1), -1, f32)
    ctx.check(ctx.L.sdso_distmap_get(ctx.h, abi.fp(m)))
    return m


def dm_add(ctx, iu, iv):
    from sdso_amd import abi
    iu, iv = np.ascontiguousarray(iu, np.int32), np.ascontiguousarray(iv, np.int32)
    ctx.check(ctx.L.sdso_distmap_add(ctx.h, len(iu), abi.ip(iu), abi.ip(iv)))


def dm_select(ctx, case):
    from sdso_amd import abi
    c = case["cand"]
    n = len(c["u"])
    keep = [abi.make_distmap_geoms(case["KRKi"], case["Kt"]), np.ascontiguousarray(case["flagged"], np.uint8)]
    S = abi.ActivateSelect()
    S.w, S.h, S.ngeom, S.n = case["w"], case["h"], len(case["KRKi"]), n
    S.geom = C.cast(keep[0], C.POINTER(abi.DistMapGeom))
    S.host_flagged = abi.bp(keep[1])
    for field, key, conv, dt in (("point_geom", "pg", abi.ip, np.int32), ("u", "u", abi.fp, f32), ("v", "v", abi.fp, f32), ("idepth_min", "idepth_min", abi.fp, f32),
                                 ("idepth_max", "idepth_max", abi.fp, f32), ("quality", "quality", abi.fp, f32), ("lastTracePixelInterval", "interval", abi.fp, f32),
                                 ("lastTraceStatus", "status", abi.bp, np.uint8), ("my_type", "my_type", abi.fp, f32)):
        a = np.ascontiguousarray(c[key], dt)
        keep.append(a)
        setattr(S, field, conv(a))
    S.currentMinActDist = float(case["min_act_dist"])
    S.minTraceQuality = float(case["min_trace_quality"])
    dec, iu, iv = np.full(n, 255, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    ns = C.c_int(-1)
    ctx.check(ctx.L.sdso_activate_select(ctx.h, C.byref(S), abi.bp(dec), abi.ip(iu), abi.ip(iv), C.byref(ns)))
    return dict(decision=dec, iu=iu, iv=iv, n_selected=ns.value)


def ref_select(ref, case, m, regrow=True):
    c = case["cand"]
    return ref.select(m, case["w"], case["h"], case["KRKi"], case["Kt"], case["flagged"], c["pg"], c["u"], c["v"], c["idepth_min"], c["idepth_max"],
                      c["quality"], c["interval"], c["status"], c["my_type"], case["min_act_dist"], case["min_trace_quality"], regrow=regrow)
