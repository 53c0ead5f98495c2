"""The window of the sdso_imm_activate tests: immature_cases.window_case traced over two non-key frames and frame 2 as key on the CPU
statement, then hosts 0, 1, 2 + frame 2's left image as a window of nf = 4 with host 0 flagged for marginalisation.

A naturally traced state does not reach every branch of activatePointsMT (no projection outside the map, no status 0, no selected
candidate that is IPS_OOB), so disjoint strided groups of the activatable points of every larger host are doctored; the state is then
installed with sdso_imm_put_host.  tests/test_activate_ref.py asserts on the CPU statement alone that every branch occurs."""
import copy
import functools

import numpy as np

import distmap_cases as DC
import distmap_ref as D
import immature_cases as Cs
import immature_ref as R
import synth

f32 = np.float32
MIN_ACT_DIST = f32(0.7)
STRIDE = 13     # > the number of doctorings: group k takes the activatable points k, k + STRIDE, ...


def _activatable(S, min_trace_quality=3.0):
    st = S["lastTraceStatus"]
    with np.errstate(all="ignore"):
        return (np.isfinite(S["idepth_max"]) & np.isin(st, (R.GOOD, R.SKIPPED, R.BADCONDITION, R.OOB)) & (S["lastTracePixelInterval"] < 8)
                & (S["quality"] > f32(min_trace_quality)) & ((S["idepth_max"] + S["idepth_min"]) > 0))


def doctor(S):
    """Every gate of STEP 2 and every exit of optimizeImmaturePoint, on disjoint groups of the activatable points of S (in place)."""
    a = np.nonzero(_activatable(S))[0]
    grp = lambda k: a[k::STRIDE]
    S["idepth_max"][grp(0)] = np.nan                                        # :850 never traced successfully
    S["lastTraceStatus"][grp(1)] = R.OUTLIER                                # :850
    S["quality"][grp(2)] = f32(3.0)                                         # exactly on the bar: `>` fails
    g = grp(3); S["lastTracePixelInterval"][g] = f32(8); S["lastTraceStatus"][g[::2]] = R.OOB      # not activatable; OOB is deleted
    g = grp(4); S["idepth_min"][g] = f32(40); S["idepth_max"][g] = f32(60)  # projects far outside the map
    g = grp(5); S["weights"][g] *= f32(1e-4); S["lastTraceStatus"][g[::2]] = R.OOB                 # Hdd below the bar: status 0, with / without OOB
    S["energyTH"][grp(6)] = np.nan                                          # status -1 by energyTH
    g = grp(7); S["idepth_min"][g] *= f32(0.05); S["idepth_max"][g] *= f32(0.1)                    # interval far off: outliers
    g = grp(8); S["idepth_min"][g] = -np.abs(S["idepth_max"][g]) - f32(0.01)                       # idepth_max + idepth_min <= 0
    S["lastTraceStatus"][grp(9)] = R.UNINITIALIZED                          # not activatable
    return S


@functools.lru_cache(maxsize=1)
def _traced():
    import pyoracle
    orc = pyoracle.load()
    case = Cs.window_case()
    hosts, frames = case["hosts"], case["frames"]
    groups = [R.add_frame(orc, h_["img"], h_["map"]) for h_ in hosts]
    for k, nonkey in ((0, True), (1, True), (2, False)):
        F = frames[k]
        R.trace(orc, [(groups[j], F["geom"][j]) for j in range(4)], F["left"], F["right"] if nonkey else None, case["K4"], case["Ki"], case["baseline"])
    return case, groups


def window(orc, doctored=True):
    """-> dict(win=the window of activate_ref.activate, seeds=(pg, u, v, idepth) of the distance map, case, empty=host 3's group)"""
    case, groups = _traced()
    groups = copy.deepcopy(groups)
    hosts, F = case["hosts"], case["frames"][2]
    K4 = case["K4"]
    if doctored:
        for S in groups[:3]:
            if len(S["u"]) >= 50:
                doctor(S)
    T = [hosts[0]["T"], hosts[1]["T"], hosts[2]["T"], F["T"]]
    affs = [(0.0, 0.0)] * 3 + [F["aff"]]
    nf = 4
    pair_R, pair_t, pair_aff = np.zeros((nf * nf, 9), f32), np.zeros((nf * nf, 3), f32), np.zeros((nf * nf, 2), f32)
    for h in range(nf):
        for t in range(nf):
            Rm, tv = synth.se3_mul(T[t], synth.se3_inv(T[h]))                    # leftToLeft = target.worldToCam * host.camToWorld
            pair_R[h * nf + t] = Rm.astype(f32).ravel(); pair_t[h * nf + t] = tv.astype(f32)
            a = np.exp(affs[t][0] - affs[h][0])                                  # AffLight::fromToVecExposure, exposures 1
            pair_aff[h * nf + t] = (a, affs[t][1] - a * affs[h][1])
    KRKi, Kt = DC.window_geoms(np.array([synth.se3_pack(x) for x in T]), tuple(float(x) for x in K4))
    fxs, fys, cxs, cys = synth.level_intrinsics(*[float(x) for x in K4], 2)
    K1 = np.array([[fxs[1], 0, cxs[1]], [0, fys[1], cys[1]], [0, 0, 1]], f32)
    K0 = np.array([[fxs[0], 0, cxs[0]], [0, fys[0], cys[0]], [0, 0, 1]], np.float64)
    KRKi[1] = K1 @ np.linalg.inv(K0).astype(f32)                                 # host 1: a pure sideways geometry (any float values do)
    Kt[1] = np.array([0.8 * fxs[1], 0, 0], f32)
    win = dict(groups=groups[:3] + [None], imgs=[hosts[0]["img"], hosts[1]["img"], hosts[2]["img"], F["left"]], flagged=np.array([1, 0, 0, 0], np.uint8),
               KRKi=KRKi, Kt=Kt, pair_R=pair_R, pair_t=pair_t, pair_aff=pair_aff, K4=K4, w=Cs.W, h=Cs.H)
    # the seeds of the map: every 7th point of hosts 0 and 1 with a finite interval, at the middle of its interval
    pg, u, v, idp = [], [], [], []
    for g in (0, 1):
        S = groups[g]
        i = np.arange(len(S["u"]))[::7]
        i = i[np.isfinite(S["idepth_max"][i]) & np.isfinite(S["idepth_min"][i])]
        pg.append(np.full(len(i), g, np.int32)); u.append(S["u"][i]); v.append(S["v"][i]); idp.append(f32(0.5) * (S["idepth_max"][i] + S["idepth_min"][i]))
    seeds = tuple(np.ascontiguousarray(np.concatenate(x)) for x in (pg, u, v, idp))
    return dict(win=win, seeds=seeds, case=case, empty=groups[3], min_act_dist=MIN_ACT_DIST)


def ref_map(c):
    """makeDistanceMap on the case's seeds -> (map float32 (h1, w1), flat list)"""
    pg, u, v, idp = c["seeds"]
    mp, _, m = D.make_distance_map(c["win"]["w"], c["win"]["h"], c["win"]["KRKi"], c["win"]["Kt"], pg, u, v, idp)
    return mp, m
