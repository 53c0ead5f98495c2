"""FullSystem::optimize as the fork compiles it (FullSystemOptimize.cpp:402-868), restated in NumPy f64 over the CPU oracle's
orc_g2o_lba_eval (bit-exact with the device edge, tests/test_g2o_factors.py::test_gpu_lba_edge_bit_exact): the reference that
sdso_g2o_lba_optimize is held to.  g2o is neither vendored nor version-pinned by the fork (CMakeLists.txt:47-58); what it decides is
restated from its published algorithm, in the form csrc/g2o_factors.hip:480-531 has for the tracker:

  graph        one pose + one photometric vertex per HOST frame, one idepth vertex per RESIDUAL, one camera vertex (:455-542); the
               target pose is a constant (dso_g2o_edge.cpp:23)
  active set   edges with level 0 after the build-time computeError (:539, initializeOptimization :587); setLevel(1) is never undone
               (dso_g2o_edge.cpp:63), and linearizeOplus returns early on level 1 / OOB / a non-finite sample (:131, :183, :194, :204)
  kernel       RobustKernelHuber on the squared norm of the 8-vector, delta = setting_huberTH = 9 (:529-531)
  LM           OptimizationAlgorithmLevenberg: lambda on EVERY diagonal before the Schur complement, computeScale over the whole
               solution, rho = (chi - chi') / (scale + 1e-3), 1/3..2/3 factor, nu doubling, up to max_trials trials
  terminate    SparseOptimizerTerminateAction: gain = (lastChi - chi) / chi on a fresh computeActiveErrors, stop at 0 <= gain < thr
  oplus        exp(d) * Twh, a += d, b += d, idepth += d, cam += d (dso_g2o_vertex.cpp:15-18, :30-40, :56-58, :100-106)

The float pair tables are formed in the library's operation order (csrc/host_math.h: Se3 product, affFromTo) so that equal double
estimates give equal tables.
"""
import ctypes as C
import math

import numpy as np

from sdso_amd import abi
import synth

HUBER = 9.0                  # setting_huberTH, settings.cpp:95
STOP_ITERATIONS, STOP_GAIN, STOP_TRIALS, STOP_RHO_ZERO, STOP_LAMBDA = range(5)

# (nf, points per keyframe, seed, iterations, left-perturbation of Twh, lambda0)
CASES = {
    "A": (5, 60, 3061, 3, 0.0, 0.1),
    "B": (3, 40, 3062, 7, 1e-3, 0.1),
    "C": (2, 40, 3063, 10, 1e-3, 0.1),
    "D": (8, 30, 3064, 3, 5e-4, 0.1),
    "E": (2, 40, 3063, 10, 1e-3, 1e-9),
    "F": (5, 60, 3061, 3, 0.0, 0.1),       # A with the doctored points of test_gpu_lba_edge_bit_exact
    "G": (3, 40, 3062, 7, 1e-3, 0.1),      # B with every point of host 1 moved out of the image: a host without an active edge
}
W_IMG, H_IMG = 640, 480


# ------------------------------------------------------------------------------------------------ the library's double math, restated
def mul3(a, b):
    """host_math.h mul(M3, M3): c_ij = a_i0 b_0j + a_i1 b_1j + a_i2 b_2j, left to right"""
    return a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :] + a[:, 2:3] * b[2:3, :]


def mulv(a, x):
    return a[:, 0] * x[0] + a[:, 1] * x[1] + a[:, 2] * x[2]


def se3_mul(A, B):
    """host_math.h operator*(Se3, Se3)"""
    return mul3(A[0], B[0]), mulv(A[0], B[1]) + A[1]


def se3_exp(xi):
    """host_math.h expSe3 (Sophus se3.hpp:406-428 through the unit quaternion)"""
    om = [float(x) for x in xi[3:6]]
    th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    th = math.sqrt(th2)
    if th < 1e-10:
        th4 = th2 * th2
        im = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4
        re = 1.0 - 0.5 * th2 + (1.0 / 384.0) * th4
    else:
        im = math.sin(0.5 * th) / th
        re = math.cos(0.5 * th)
    w, x, y, z = re, im * om[0], im * om[1], im * om[2]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w /= n; x /= n; y /= n; z /= n
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Om = synth.hat(om)
    Om2 = mul3(Om, Om)
    if th < 1e-10:
        V = R
    else:
        a = (1.0 - math.cos(th)) / (th * th)
        b = (th - math.sin(th)) / (th * th * th)
        V = np.eye(3) + a * Om + b * Om2
    return R, mulv(V, np.asarray(xi[0:3], np.float64))


def pair_tables(case, Twh, aff):
    """dso_g2o_edge.cpp:25-28 and :86-91, cast to float"""
    nf = case["nf"]
    pR = np.zeros((nf * nf, 9), np.float32); pt = np.zeros((nf * nf, 3), np.float32); pab = np.zeros((nf * nf, 2), np.float32)
    for h in range(nf):
        for t in range(nf):
            T = se3_mul(case["Ttw"][t], Twh[h])
            pR[h * nf + t] = T[0].astype(np.float32).ravel(); pt[h * nf + t] = T[1].astype(np.float32)
            ef, et = float(case["ab_exposure"][h]), float(case["ab_exposure"][t])
            if ef == 0 or et == 0:
                ef = et = 1.0
            a = math.exp(case["target_aff"][t][0] - aff[h][0]) * et / ef
            pab[h * nf + t] = (a, case["target_aff"][t][1] - a * aff[h][1])
    return pR, pt, pab


# ------------------------------------------------------------------------------------------------ cases
def build_case(name):
    nf, ppk, seed, iters, pert, lam0 = CASES[name]
    wk = (nf, ppk, seed)
    if wk not in _windows:
        _windows[wk] = synth.ba_window(w=W_IMG, h=H_IMG, nf=nf, pts_per_kf=ppk, seed=seed)
    win = _windows[wk]
    rp = win["res_point"]
    rs = np.random.RandomState(seed + 1)
    Twh = []
    for h in range(nf):
        d = rs.randn(6) * pert
        Twh.append(synth.se3_mul(synth.se3_exp(d), synth.se3_inv(win["poses"][h])))
    c = dict(name=name, nf=nf, nr=len(rp), w=W_IMG, h=H_IMG, win=win, iterations=iters, lambda_init=lam0,
             Ttw=[(np.array(p[0], np.float64), np.array(p[1], np.float64)) for p in win["poses"]],
             target_aff=[(float(a), float(b)) for a, b in win["affs"]], ab_exposure=win["ab_exposure"].copy(),
             host_b0=np.array([win["affs"][h][1] for h in range(nf)], np.float64), frameEnergyTH=win["frameEnergyTH"].copy(),
             host=np.ascontiguousarray(win["host"][rp], np.int32), target=np.ascontiguousarray(win["res_target"], np.int32),
             u=np.ascontiguousarray(win["u"][rp]).copy(), v=np.ascontiguousarray(win["v"][rp]).copy(),
             color=np.ascontiguousarray(win["color"][rp]), weights=np.ascontiguousarray(win["weights"][rp]),
             Twh=Twh, host_aff=[(float(a), float(b)) for a, b in win["affs"]], cam=np.array([float(x) for x in win["K"]], np.float64),
             idepth=np.ascontiguousarray(win["idepth"][rp], np.float64).copy())
    if name == "F":      # tests/test_g2o_factors.py::test_gpu_lba_edge_bit_exact
        r7 = np.random.RandomState(7)
        k = r7.choice(c["nr"], 60, replace=False)
        c["u"][k[:15]] = r7.uniform(-30, 3, 15).astype(np.float32); c["v"][k[15:30]] = r7.uniform(470, 520, 15).astype(np.float32)
        c["idepth"][k[30:45]] *= r7.uniform(20, 200, 15)
        c["idepth"][k[45:60]] *= -r7.uniform(20, 200, 15)
        c["frameEnergyTH"][1] = 40.0
    if name == "G":
        c["u"][c["host"] == 1] = -2000.0
    return c


_cache = {}
_windows = {}


def case(name):
    """built once, shared, never modified"""
    if name not in _cache:
        _cache[name] = build_case(name)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the edge, through the oracle
def oracle_eval(orc, c, Twh, aff, cam, idepth):
    nf, nr = c["nf"], c["nr"]
    pR, pt, pab = pair_tables(c, Twh, aff)
    S = abi.G2oLba()
    S.nf, S.nr, S.w, S.h = nf, nr, c["w"], c["h"]
    S.cam[:] = [float(x) for x in cam]
    idp = np.ascontiguousarray(idepth, np.float64)
    dI = [np.ascontiguousarray(p[0], np.float32) for p in c["win"]["pyrs"]]
    ptrs = (abi.c_float_p * nf)(*[abi.fp(a) for a in dI])
    S.dI = C.cast(ptrs, C.POINTER(abi.c_float_p))
    S.pair_R, S.pair_t, S.pair_ab = abi.fp(pR), abi.fp(pt), abi.fp(pab)
    S.host_b0, S.frameEnergyTH = abi.dp(c["host_b0"]), abi.fp(c["frameEnergyTH"])
    S.host, S.target, S.u, S.v = abi.ip(c["host"]), abi.ip(c["target"]), abi.fp(c["u"]), abi.fp(c["v"])
    S.idepth, S.color, S.weights = abi.dp(idp), abi.fp(c["color"]), abi.fp(c["weights"])
    o = dict(error=np.zeros((nr, 8)), J=np.zeros((nr, 8, 13)), state=np.zeros(nr, np.uint8), energy=np.zeros((nr, 2), np.float32),
             cpt=np.zeros((nr, 3), np.float32), ih=np.zeros(nr, np.float32), lvl=np.zeros(nr, np.uint8), tables=(pR, pt, pab))
    assert orc.orc_g2o_lba_eval(C.byref(S), abi.dp(o["error"]), abi.dp(o["J"]), abi.bp(o["state"]), abi.fp(o["energy"]), abi.fp(o["cpt"]),
                                abi.fp(o["ih"]), abi.bp(o["lvl"])) == 0
    return o


def robust_chi2(o, active):
    e2 = (o["error"] ** 2).sum(1)
    rho0 = np.where(e2 <= HUBER * HUBER, e2, 2 * np.sqrt(e2) * HUBER - HUBER * HUBER)
    return float(rho0[active].sum())


# ------------------------------------------------------------------------------------------------ the loop
def optimize(orc, c, max_iterations=None, lambda_init=None, gain_threshold=1e-3, max_trials=10, evaluate=None):
    """`evaluate(orc, c, Twh, aff, cam, idepth)`: the edge; oracle_eval unless tools/time_g2o_lba.py hands in sdso_g2o_lba_eval"""
    oracle_eval = evaluate or globals()["oracle_eval"]
    nf, nr = c["nf"], c["nr"]
    max_iterations = c["iterations"] if max_iterations is None else max_iterations
    lambda_init = c["lambda_init"] if lambda_init is None else lambda_init
    Twh = [(T[0].copy(), T[1].copy()) for T in c["Twh"]]
    aff = [tuple(a) for a in c["host_aff"]]
    cam = c["cam"].copy()
    idepth = c["idepth"].copy()
    host = c["host"]

    o = oracle_eval(orc, c, Twh, aff, cam, idepth)            # the build-time computeError, :539
    level = o["lvl"].copy()
    active = level == 0
    hosts = [h for h in range(nf) if np.any(active & (host == h))]
    slot = {h: i for i, h in enumerate(hosts)}
    nh = len(hosts)
    n = 8 * nh + 4
    chi = robust_chi2(o, active)
    res = dict(iterations=0, trials=[], lambdas=[], chi2=[], rhos=[], gains=[], stop=STOP_ITERATIONS, n_active=int(active.sum()), active=active.copy(),
               ih=np.zeros(nr, np.float32), accepted=0, rejected=0)
    PCOLS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12]
    lam, ni, last_chi = 0.0, 2.0, 0.0
    stop, ok = False, True
    it = 0
    while it < max_iterations and not stop and ok and nh > 0:
        # linearizeOplus + the quadratic form at the current estimate
        o = oracle_eval(orc, c, Twh, aff, cam, idepth)
        level |= o["lvl"]
        J = o["J"].copy()
        jz = (~active) | (level != 0)
        J[jz] = 0
        res["ih"] = np.where(jz, np.float32(0), o["ih"]).astype(np.float32)
        e = o["error"]
        e2 = (e ** 2).sum(1)
        rho1 = np.where(e2 <= HUBER * HUBER, 1.0, HUBER / np.sqrt(np.maximum(e2, 1e-300)))
        rho1 = np.where(active, rho1, 0.0)
        Jp, jd = J[:, :, PCOLS], J[:, :, 8]
        H = np.zeros((n, n)); b = np.zeros(n)
        w = rho1[:, None] * np.einsum("rki,rk->ri", Jp, jd)
        hll = rho1 * (jd * jd).sum(1)
        bl = -rho1 * (jd * e).sum(1)
        idx_of = {}
        for h in hosts:
            m = active & (host == h)
            ix = np.array([8 * slot[h] + k for k in range(8)] + [8 * nh + k for k in range(4)])
            idx_of[h] = ix
            H[np.ix_(ix, ix)] += np.einsum("r,rki,rkj->ij", rho1[m], Jp[m], Jp[m])
            b[ix] -= np.einsum("r,rki,rk->i", rho1[m], Jp[m], e[m])
        current_chi = chi
        if it == 0:
            lam, ni = lambda_init, 2.0
        rho, qmax = 0.0, 0
        while True:
            d = hll + lam
            inv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
            Hr = H + lam * np.eye(n); br = b.copy()
            for h in hosts:
                m = active & (host == h)
                ix = idx_of[h]
                Hr[np.ix_(ix, ix)] -= np.einsum("r,ri,rj->ij", inv[m], w[m], w[m])
                br[ix] -= np.einsum("r,ri,r->i", inv[m], w[m], bl[m])
            try:
                x = np.linalg.solve(Hr, br)
                solved = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x = np.zeros(n); solved = False
            xe = np.zeros((nr, 12))                                                   # the 12 increments each edge sees
            for h in hosts:
                xe[host == h] = x[idx_of[h]]
            xl = np.where(active, (bl - (w * xe).sum(1)) * inv, 0.0)
            scale = float((x * (lam * x + b)).sum() + (xl * (lam * xl + bl))[active].sum())
            Twh_t = list(Twh); aff_t = list(aff)
            for h in hosts:
                xh = x[8 * slot[h]: 8 * slot[h] + 8]
                Twh_t[h] = se3_mul(se3_exp(xh[:6]), Twh[h])
                aff_t[h] = (aff[h][0] + xh[6], aff[h][1] + xh[7])
            cam_t = cam + x[8 * nh:]
            idepth_t = idepth + xl
            ot = oracle_eval(orc, c, Twh_t, aff_t, cam_t, idepth_t)
            level |= ot["lvl"]
            temp_chi = robust_chi2(ot, active) if solved else 1.7976931348623157e308
            rho = (current_chi - temp_chi) / (scale + 1e-3)
            res["rhos"].append(rho)
            if rho > 0 and math.isfinite(temp_chi):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
                Twh, aff, cam, idepth = Twh_t, aff_t, cam_t, idepth_t
                res["accepted"] += 1
            else:
                lam *= ni
                ni *= 2
                res["rejected"] += 1
                if not math.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < max_trials):
                break
        if not math.isfinite(lam):
            ok = False; res["stop"] = STOP_LAMBDA
        elif rho == 0:
            ok = False; res["stop"] = STOP_RHO_ZERO
        elif qmax == max_trials:
            ok = False; res["stop"] = STOP_TRIALS
        o = oracle_eval(orc, c, Twh, aff, cam, idepth)          # terminate action: computeActiveErrors at the current estimate
        level |= o["lvl"]
        chi = robust_chi2(o, active)
        res["trials"].append(qmax); res["lambdas"].append(lam); res["chi2"].append(chi)
        res["iterations"] += 1
        if it == 0:
            last_chi = chi
        else:
            gain = (last_chi - chi) / chi
            res["gains"].append(gain)
            last_chi = chi
            if 0 <= gain < gain_threshold:
                stop = True
                if ok:
                    res["stop"] = STOP_GAIN
        it += 1
    res.update(Twh=Twh, host_aff=aff, cam=cam, idepth=idepth, chi2_final=chi, state=o["state"], energy=o["energy"], cpt=o["cpt"], level=level,
               tables=o["tables"], hosts=hosts,
               rmse=np.sqrt(np.float32(chi / (8.0 * nr))) if nr else np.float32(0))
    return res


_results = {}


def reference(orc, name):
    """the reference run of a case: computed once, shared, never modified"""
    if name not in _results:
        _results[name] = optimize(orc, case(name))
    return _results[name]


# ------------------------------------------------------------------------------------------------ the C-ABI call
def make_call(c, frame_slots, max_iterations=None, lambda_init=None, gain_threshold=1e-3, max_trials=10):
    """(W, P, S, out, arrays) for sdso_g2o_lba_optimize on case c; `arrays` keeps every buffer alive and is how the results are read"""
    nf, nr = c["nf"], c["nr"]
    a = dict(frame_slot=np.ascontiguousarray(frame_slots, np.int32), ab_exposure=np.ascontiguousarray(c["ab_exposure"], np.float32),
             host_b0=np.ascontiguousarray(c["host_b0"], np.float64), frameEnergyTH=np.ascontiguousarray(c["frameEnergyTH"], np.float32),
             host=np.ascontiguousarray(c["host"], np.int32), target=np.ascontiguousarray(c["target"], np.int32),
             u=np.ascontiguousarray(c["u"], np.float32), v=np.ascontiguousarray(c["v"], np.float32),
             color=np.ascontiguousarray(c["color"], np.float32), weights=np.ascontiguousarray(c["weights"], np.float32),
             idepth=np.ascontiguousarray(c["idepth"], np.float64).copy(),
             state=np.full(nr, 77, np.uint8), energy=np.zeros((nr, 2), np.float32), cpt=np.zeros((nr, 3), np.float32),
             level=np.full(nr, 77, np.uint8), ih=np.full(nr, -1, np.float32), active=np.full(nr, 77, np.uint8))
    a["Ttw"] = (abi.SE3 * nf)(*[abi.SE3.from_Rt(*T) for T in c["Ttw"]])
    a["Twh"] = (abi.SE3 * nf)(*[abi.SE3.from_Rt(*T) for T in c["Twh"]])
    a["target_aff"] = (abi.Aff * nf)(*[abi.Aff(*x) for x in c["target_aff"]])
    a["host_aff"] = (abi.Aff * nf)(*[abi.Aff(*x) for x in c["host_aff"]])
    W = abi.G2oLbaWindow()
    W.nf, W.nr, W.w, W.h = nf, nr, c["w"], c["h"]
    W.frame_slot = abi.ip(a["frame_slot"]); W.Ttw = a["Ttw"]; W.target_aff = a["target_aff"]
    W.ab_exposure = abi.fp(a["ab_exposure"]); W.host_b0 = abi.dp(a["host_b0"]); W.frameEnergyTH = abi.fp(a["frameEnergyTH"])
    W.host, W.target, W.u, W.v = abi.ip(a["host"]), abi.ip(a["target"]), abi.fp(a["u"]), abi.fp(a["v"])
    W.color, W.weights = abi.fp(a["color"]), abi.fp(a["weights"])
    S = abi.G2oLbaState()
    S.Twh = a["Twh"]; S.host_aff = a["host_aff"]; S.cam[:] = [float(x) for x in c["cam"]]; S.idepth = abi.dp(a["idepth"])
    P = abi.G2oLbaOpt()
    P.max_iterations = c["iterations"] if max_iterations is None else max_iterations
    P.lambda_init = c["lambda_init"] if lambda_init is None else lambda_init
    P.gain_threshold, P.max_trials = gain_threshold, max_trials
    out = abi.G2oLbaResult()
    out.state, out.energy, out.centerProjectedTo = abi.bp(a["state"]), abi.fp(a["energy"]), abi.fp(a["cpt"])
    out.edge_level, out.idepth_hessian, out.active = abi.bp(a["level"]), abi.fp(a["ih"]), abi.bp(a["active"])
    return W, P, S, out, a


def estimates(S, a, nf):
    """the estimates a call left behind, as the reference has them"""
    Twh = [S.Twh[h].Rt() for h in range(nf)]
    return dict(Twh=[(np.array(R, np.float64), np.array(t, np.float64)) for R, t in Twh], host_aff=[(S.host_aff[h].a, S.host_aff[h].b) for h in range(nf)],
                cam=np.array(S.cam[:], np.float64), idepth=a["idepth"].copy())
