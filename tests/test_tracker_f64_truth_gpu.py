"""The coarse tracker's evaluation (k_track_eval + k_track_finalize, csrc/tracker_eval.hip) against an f64 truth of calcRes + calcGSSSE, at
the shapes the batched kernel takes in production.

The truth: the oracle's per-point terms (calcRes' buf_warped: idepth, u, v, dx, dy, residual, weight, refColor of every warped
point) are turned into calcGSSSE's 9-vector J and summed as J_w J^T in float64; 1/n_warped (padded) and SCALE_* are applied as
k_track_finalize applies them.  E is the f64 sum of the per-point energies plus nSat * maxEnergy, the flow indicators are f64 sums
over the level-0 points with i % 32 == 0.  The per-point terms themselves are checked against a plain f64 restatement (projection,
bilinear sample, Huber) so the truth does not rest on the oracle alone.

Errors are whitened: H by sqrt(diag H) on both sides, b by sqrt(H_rr * c) with c = sum w r^2 / n (the augmented system's own
diagonal, |b_r| <= sqrt(H_rr c)), E and the flow indicators relative to their size.

Measured on MI355X (256 CUs), largest value over every problem of the parametrisation (single evaluations, the batches, the LM's
final poses), device / CPU float oracle:
  H whitened          3.3e-7 / 7.0e-7     bar 1e-6
  b whitened          1.2e-7 / 3.1e-7     bar 4e-7
  E relative          2.2e-7 / 5.4e-6     bar 7e-7
  flow indicators     6.3e-6 / 6.3e-6     bar 2e-5  (the per-point shift terms, bit-identical on both paths, cancel in float: the
                                                     error is theirs, not the sum's)
Every batch's device maximum of H, b and E is also held to NOISE_FACTOR x the CPU path's own maximum (measured 0.03..0.5x; the LM's final
poses 1.1x for H).  The per-point restatement: no term further from the f64 value than 0.3 of its tolerance; 59 of 174 201 points within
float noise of a bounds / cut-off threshold are left out of the inlier comparison."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
from sdso_amd import abi
import synth

pytestmark = pytest.mark.gpu

W0, H0 = 1232, 368
TRK_BLOCK, TRK_UNROLL = 256, 4          # the constants of those names in tracker_eval.hip
LM_BLOCK, LM_UNROLL, LM_MAXG = 512, 4, 8  # LM_BLOCK_THREADS / LM_UNROLL in tracker_lm_core.h, LM_MAXG in tracker_lm.hip
SC = np.array([synth.SCALE_XI_ROT] * 3 + [synth.SCALE_XI_TRANS] * 3 + [synth.SCALE_A, synth.SCALE_B], np.float64)
NFRAMES = 128                           # bench.py TrackerWorkload: 128 frames x 5 levels
SIZES = (0, 1, 255, 256, 257, 1024, 1025, 4097, 12000, 20000)   # level-0 templates
FRAME0, REF0, REFSUB0 = 500, 600, 610   # slots of this module (the session context is shared with the other test files)

# bars: about 3x the largest device error measured (docstring)
TOL_H, TOL_B, TOL_E, TOL_F = 1e-6, 4e-7, 7e-7, 2e-5
NOISE_FACTOR = 4.0                      # device error <= this x the CPU float oracle's error to the same truth (+ a floor)


def choose_gx(n_cu, nprob, maxn):
    """choose_gx (tracker_eval_api.hip) — workgroups per problem of a batched k_track_eval launch"""
    if maxn <= 0:
        return 1
    by_points = (maxn + TRK_BLOCK - 1) // TRK_BLOCK
    target = (n_cu * 8 + nprob - 1) // nprob
    return max(1, min(by_points, target))


def lane_trips(n, gx):
    """trips of track_accumulate's lane loop (tracker_eval.hip): TRK_UNROLL points per lane and trip, gx * TRK_BLOCK lanes"""
    return -(-n // (TRK_UNROLL * TRK_BLOCK * gx)) if n > 0 else 0


def subset(pc_l, n):
    """n template points spread evenly over the level (the template is in row order: a prefix would be the top of the image only)"""
    m = len(pc_l["u"])
    assert n <= m
    idx = np.unique(np.round(np.linspace(0, m - 1, n)).astype(np.int64)) if n else np.zeros(0, np.int64)
    assert len(idx) == n
    return {k: np.ascontiguousarray(v[idx]) for k, v in pc_l.items()}


EMPTY = dict(u=np.zeros(0, np.float32), v=np.zeros(0, np.float32), idepth=np.zeros(0, np.float32), color=np.zeros(0, np.float32))


# ------------------------------------------------------------------ the f64 truth
def truth(pc_l, ev, reso, nwo, masko, buf):
    """(1) calcGSSSE + calcRes' sums in float64 from the oracle's per-point terms"""
    idp, u, v, dxi, dyi, r, w, col = buf.astype(np.float64)
    fx, fy = float(ev.fx), float(ev.fy)
    dx, dy = dxi * fx, dyi * fy
    J = np.empty((nwo, 9))
    J[:, 0] = idp * dx
    J[:, 1] = idp * dy
    J[:, 2] = 0.0 - idp * (u * dx + v * dy)
    J[:, 3] = 0.0 - ((u * v) * dx + dy * (1.0 + v * v))
    J[:, 4] = (u * v) * dy + dx * (1.0 + u * u)
    J[:, 5] = u * dy - v * dx
    J[:, 6] = float(ev.affLL[0]) * (float(ev.ref_b0) - col)
    J[:, 7] = -1.0
    J[:, 8] = r
    A = (J * w[:, None]).T @ J
    inv_n = float(np.float32(1) / np.float32(nwo)) if nwo > 0 else 0.0      # k_track_finalize: float 1 / npad, then double
    H = A[:8, :8] * inv_n * SC[None, :] * SC[:, None]
    b = A[:8, 8] * inv_n * SC
    c = A[8, 8] * inv_n
    hu, cu = np.float32(ev.huberTH), np.float32(ev.cutoffTH)
    maxE = float(np.float32(np.float32(np.float32(2) * hu) * cu) - np.float32(hu * hu))
    nE = int(reso[1])
    nsat = nE - int(masko.sum())
    E = float(np.sum(w * r * r * (2.0 - w))) + nsat * maxE
    f2 = f4 = 0.0
    if ev.lvl == 0:
        sel = np.arange(len(pc_l["u"])) % 32 == 0
        x, y, d = [pc_l[k][sel].astype(np.float64) for k in ("u", "v", "idepth")]
        Ki, RKi = np.array(ev.Ki, np.float64).reshape(3, 3), np.array(ev.RKi, np.float64).reshape(3, 3)
        t = np.array(ev.t, np.float64)
        X = np.stack([x, y, np.ones_like(x)])
        kp, rp = Ki @ X, RKi @ X
        cx, cy = float(ev.cx), float(ev.cy)

        def shift(p):
            return (fx * (p[0] / p[2]) + cx - x) ** 2 + (fy * (p[1] / p[2]) + cy - y) ** 2
        td = t[:, None] * d[None, :]
        num = 2.0 * sel.sum()
        f2 = float(np.sum(shift(kp + td) + shift(kp - td))) / (num + 0.1)
        f4 = float(np.sum(shift(rp + td) + shift(rp - td))) / (num + 0.1)
    return dict(H=H, b=b, c=c, E=E, f2=f2, f4=f4, nw=nwo, nE=nE, res5=reso[5])


def restate_points(pc_l, img, ev):
    """(2) calcRes per point in plain f64: projection, bounds, bilinear sample, Huber, cutoff.  Returns the warped fields of every
    point (WARPED_FIELDS order), the inlier and bounds decisions, the distance of every point's decisions to their thresholds and the
    tolerance of its image samples."""
    x, y, d, col = [pc_l[k].astype(np.float64) for k in ("u", "v", "idepth", "color")]
    RKi = np.array(ev.RKi, np.float64).reshape(3, 3)
    t = np.array(ev.t, np.float64)
    pt = RKi @ np.stack([x, y, np.ones_like(x)]) + t[:, None] * d[None, :]
    u, v = pt[0] / pt[2], pt[1] / pt[2]
    Ku, Kv = float(ev.fx) * u + float(ev.cx), float(ev.fy) * v + float(ev.cy)
    nid = d / pt[2]
    wl, hl = ev.w, ev.h
    inb = (Ku > 2) & (Kv > 2) & (Ku < wl - 3) & (Kv < hl - 3) & (nid > 0)
    pos_margin = np.min(np.abs(np.stack([Ku - 2, Kv - 2, Ku - (wl - 3), Kv - (hl - 3)])), axis=0)
    kx = np.where(inb, Ku, 2.5)
    ky = np.where(inb, Kv, 2.5)
    ix, iy = np.floor(kx).astype(np.int64), np.floor(ky).astype(np.int64)
    ax, ay = kx - ix, ky - iy
    I = img.astype(np.float64)
    hit = ((1 - ax) * (1 - ay))[:, None] * I[iy, ix] + (ax * (1 - ay))[:, None] * I[iy, ix + 1] + \
          ((1 - ax) * ay)[:, None] * I[iy + 1, ix] + (ax * ay)[:, None] * I[iy + 1, ix + 1]
    resid = hit[:, 0] - (float(ev.affLL[0]) * col + float(ev.affLL[1]))
    ar = np.abs(resid)
    hu, cu = float(ev.huberTH), float(ev.cutoffTH)
    hw = np.where(ar < hu, 1.0, hu / np.maximum(ar, 1e-300))
    inl = inb & np.isfinite(hit[:, 0]) & (ar <= cu)
    # the float path samples at a position a few ulps of K* away (<= 2.5e-4 px at 1232 px): a sample moves by that times the spread of its taps
    taps = np.stack([I[iy, ix], I[iy, ix + 1], I[iy + 1, ix], I[iy + 1, ix + 1]])
    spread = taps.max(axis=0) - taps.min(axis=0)
    samp_tol = 5e-4 * spread + 1e-6 * (np.abs(hit) + 1.0)
    r_margin = np.abs(ar - cu) / (samp_tol[:, 0] + 1e-6 * np.abs(col))
    fields = np.stack([nid, u, v, hit[:, 1], hit[:, 2], resid, hw, col])
    return fields, inl, inb, pos_margin, r_margin, samp_tol


# ------------------------------------------------------------------ comparison
def errors(got, tr):
    """whitened / relative distances of one evaluation (H 8x8, b 8, res 6) from its truth"""
    H, b, res = got
    if tr["nw"] == 0:
        return dict(H=float(np.abs(H).max()), b=float(np.abs(b).max()), E=abs(res[0] - tr["E"]) / max(tr["E"], 1e-30), F=0.0)
    d = np.sqrt(np.abs(np.diag(tr["H"])))
    dd = np.outer(d, d)
    eH = float(np.max(np.abs(H - tr["H"]) / np.where(dd > 0, dd, 1.0)))
    sb = d * math.sqrt(max(tr["c"], 0.0))
    eb = float(np.max(np.abs(b - tr["b"]) / np.where(sb > 0, sb, 1.0)))
    eE = abs(res[0] - tr["E"]) / tr["E"] if tr["E"] > 0 else abs(res[0])
    eF = 0.0
    if tr["f2"] > 0:
        eF = max(abs(res[2] - tr["f2"]) / tr["f2"], abs(res[4] - tr["f4"]) / tr["f4"])
    return dict(H=eH, b=eb, E=eE, F=eF)


class Stats:
    def __init__(self):
        self.dev = dict(H=0.0, b=0.0, E=0.0, F=0.0)
        self.cpu = dict(H=0.0, b=0.0, E=0.0, F=0.0)

    def add(self, dev, cpu):
        for k in self.dev:
            self.dev[k] = max(self.dev[k], dev[k])
            self.cpu[k] = max(self.cpu[k], cpu[k])

    def __repr__(self):
        return " ".join("%s dev %.2e cpu %.2e" % (k, self.dev[k], self.cpu[k]) for k in self.dev)


def check_problem(tag, H, b, res, nw, exp, stats):
    """one device result against its problem's truth; the bookkeeping bit-exact against the oracle"""
    tr, Ho, bo, reso, nwo = exp["truth"], exp["H"], exp["b"], exp["res"], exp["nw"]
    assert nw == nwo and res[1] == reso[1], (tag, nw, nwo, res[1], reso[1])
    assert res[5] == reso[5] or (np.isnan(res[5]) and np.isnan(reso[5])), tag
    assert res[3] == 0.0
    e_dev = errors((H.reshape(8, 8), b, res), tr)
    e_cpu = errors((Ho, bo, reso), tr)
    stats.add(e_dev, e_cpu)
    assert e_dev["H"] <= TOL_H and e_dev["b"] <= TOL_B and e_dev["E"] <= TOL_E and e_dev["F"] <= TOL_F, (tag, e_dev, e_cpu)
    return e_dev, e_cpu


def assert_not_noisier(stats, tag):
    print("\n%s: %r" % (tag, stats))
    for k in ("H", "b", "E"):
        assert stats.dev[k] <= NOISE_FACTOR * stats.cpu[k] + 2e-7, (tag, k, stats)


# ------------------------------------------------------------------ the scene: the bench's 128 noisy frames and the templates
class Scene:
    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle
        L = ctx.L
        prob = synth.tracker_problem(w=W0, h=H0, npts=2000, seed=2002)                  # bench.py TrackerWorkload, rank 0
        big = synth.tracker_problem(w=W0, h=H0, npts=6000, seed=2003)                   # level 0: ~27 500 points
        self.prob, self.big = prob, big
        self.levels = prob["levels"]
        self.prm = helpers.track_params(prob)
        ctx.set_ref(REF0, prob["pc"])
        self.base = np.ascontiguousarray(prob["pyr_new"][0][..., 0])
        rs = np.random.RandomState(77)
        for f in range(NFRAMES):                                                         # bench.py: the same noise, the same order
            img = self.frame_image(rs)
            ctx.check(L.sdso_make_pyramid(ctx.h, FRAME0 + f, W0, H0, abi.fp(img)))
        self.probs = []                                                                  # unique problems: (ref slot, frame, lvl, pc_l, ev)
        for f in range(NFRAMES):
            for lvl in range(self.levels):
                xi = np.array([0.02, -0.01, 0.35, 0.004, -0.006, 0.002]) + rs.normal(0, 2e-3, 6)
                self.probs.append((REF0, f, lvl, prob["pc"][lvl], self.make_eval(lvl, xi, (0.02, 1.0))))
        self.nbench = len(self.probs)
        # level-0 templates of SIZES points (from the denser template), three frames each
        self.sub = {}
        rs2 = np.random.RandomState(31)
        for k, n in enumerate(SIZES):
            pcs = [subset(big["pc"][0], n)] + [EMPTY] * (self.levels - 1)
            ctx.set_ref(REFSUB0 + k, pcs)
            self.sub[n] = []
            for f in (0, 57, 127):
                xi = np.array([0.02, -0.01, 0.35, 0.004, -0.006, 0.002]) + rs2.normal(0, 2e-3, 6)
                self.sub[n].append(len(self.probs))
                self.probs.append((REFSUB0 + k, f, 0, pcs[0], self.make_eval(0, xi, (0.02, 1.0))))
        self.exp = [None] * len(self.probs)
        self._oracle_all()

    def frame_image(self, rs):
        return np.clip(self.base + rs.uniform(-1.0, 1.0, self.base.shape).astype(np.float32), 0, 255).astype(np.float32)

    def make_eval(self, lvl, xi, aff, repeat=1.0):
        ev = abi.TrackEval()
        self.ctx.L.sdso_track_make_eval(C.byref(self.prm), lvl, C.byref(abi.SE3.from_Rt(*synth.se3_exp(xi))), C.byref(abi.Aff(*aff)),
                                        repeat, C.byref(ev))
        return ev

    def _oracle_all(self):
        by_frame = {}
        for i, p in enumerate(self.probs):
            by_frame.setdefault(p[1], []).append(i)
        rs = np.random.RandomState(77)
        for f in range(NFRAMES):
            img = self.frame_image(rs)
            if f not in by_frame:
                continue
            pyr = synth.make_pyramid(img, self.levels)
            if f in (0, NFRAMES - 1):                       # the host pyramid the oracle reads is the one the device built
                for l in range(self.levels):
                    out = np.zeros_like(pyr[l])
                    self.ctx.check(self.ctx.L.sdso_download_pyramid_level(self.ctx.h, FRAME0 + f, l, abi.fp(out)))
                    assert np.array_equal(out, pyr[l]), (f, l)
            for i in by_frame[f]:
                ref, _, lvl, pc_l, ev = self.probs[i]
                Ho, bo, reso, nwo, masko, buf = helpers.oracle_eval_warped(self.oracle, pc_l, pyr[lvl], ev)
                self.exp[i] = dict(H=Ho, b=bo, res=reso, nw=nwo, mask=masko, truth=truth(pc_l, ev, reso, nwo, masko, buf))
                if f in (0, 57) or i >= self.nbench:      # (2) on a sample: every level of two frames and every template size
                    self.exp[i]["restated"] = restate_check(pc_l, pyr[lvl], ev, masko, buf)

    def slots(self, idx):
        refs = np.array([self.probs[i][0] for i in idx], np.int32)
        frames = np.array([FRAME0 + self.probs[i][1] for i in idx], np.int32)
        evs = (abi.TrackEval * len(idx))(*[self.probs[i][4] for i in idx])
        return refs, frames, evs

    def maxn(self, idx):
        return max(len(self.probs[i][3]["u"]) for i in idx)

    def release(self):
        for f in range(NFRAMES):
            self.ctx.L.sdso_release_pyramid(self.ctx.h, FRAME0 + f)
        for r in [REF0] + [REFSUB0 + k for k in range(len(SIZES))]:
            self.ctx.L.sdso_track_release_ref(self.ctx.h, r)


def restate_check(pc_l, img, ev, masko, buf):
    """(2): the oracle's warped points against the f64 restatement; returns (points excluded as on a threshold, points)"""
    fields, inl, inb, pos_m, r_m, samp_tol = restate_points(pc_l, img, ev)
    edge = (pos_m < 2e-3) | (inb & (r_m < 1.0))
    ok = ~edge
    assert np.array_equal(masko[ok].astype(bool), inl[ok]), "inlier decisions differ away from their thresholds"
    sel = masko.astype(bool)
    nin = int(sel.sum())
    got = buf[:, :nin].astype(np.float64)
    ref = fields[:, sel]
    keep = ok[sel]
    rtol = samp_tol[sel, 0] + 1e-6 * np.abs(ref[7])
    stol = {"dx": samp_tol[sel, 1], "dy": samp_tol[sel, 2], "residual": rtol,
            "weight": 1e-6 * ref[6] + ref[6] * rtol / np.maximum(np.abs(ref[5]), float(ev.huberTH))}   # huber / |r| moves with r
    for k, name in enumerate(helpers.WARPED_FIELDS):
        a, e = got[k, keep], ref[k, keep]
        if not len(a):
            continue
        # float tolerance: a few ulps of the value (of the field's largest value where the float expression cancels, u and v near 0);
        # the image samples: what the float path's sampling position leaves (restate_points)
        tol = stol[name][keep] if name in stol else 1e-6 * (np.abs(e) + np.abs(e).max())
        bad = np.abs(a - e) > tol
        assert not bad.any(), (name, int(bad.sum()), float(np.max(np.abs(a - e))))
    return int(edge.sum()), len(masko)


@pytest.fixture(scope="module")
def n_cu():
    """the CU count choose_gx sees (ctx.hip: hipDeviceProp.multiProcessorCount), from torch — in a child process: torch carries a HIP
    runtime of its own, which does not find the device once the library's runtime holds it in this process"""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120, check=True)
    return int(out.stdout.split()[-1])


@pytest.fixture(scope="module")
def scene(gpu_ctx, oracle):
    s = Scene(gpu_ctx, oracle)
    yield s
    s.release()


def batches(scene, n_cu):
    """the problem lists of the batched tests: name -> indices into scene.probs"""
    bench = list(range(scene.nbench))
    tmpl = [i for n in SIZES for i in scene.sub[n]]
    rs = np.random.RandomState(5)
    pool = bench + tmpl
    n2 = max(1100, 4 * n_cu + 76)        # ceil(8 n_cu / n) == 2
    n1 = max(2100, 8 * n_cu + 52)        # == 1

    def cycled(n):
        out = []
        while len(out) < n:
            out += list(rs.permutation(pool))
        return out[:n]
    ragged = [scene.sub[n][k] for k in range(2) for n in SIZES]
    return {"bench640": bench, "bench641": bench + [scene.sub[12000][0]], "gx2": cycled(n2), "gx1": cycled(n1), "ragged": ragged}


def run_batch(ctx, scene, idx):
    refs, frames, evs = scene.slots(idx)
    n = len(idx)
    L = ctx.L
    ctx.check(L.sdso_track_batch_prepare(ctx.h, n, abi.ip(refs), abi.ip(frames), evs))
    ctx.check(L.sdso_track_batch_enqueue(ctx.h))
    H = np.zeros((n, 64)); b = np.zeros((n, 8)); res = np.zeros((n, 6)); nw = np.zeros(n, np.int32)
    ctx.check(L.sdso_track_batch_fetch(ctx.h, abi.dp(H), abi.dp(b), abi.dp(res), abi.ip(nw)))
    return H, b, res, nw


# ------------------------------------------------------------------ tests
def test_shapes_reach_every_form(scene, n_cu):
    """the parametrisation below reaches gx 1, 2, 4 and >= 8 of choose_gx and lane loops of several trips — a shape that stops covering
    its form fails here instead of passing quietly"""
    forms = {}
    for name, idx in batches(scene, n_cu).items():
        gx = choose_gx(n_cu, len(idx), scene.maxn(idx))
        forms[name] = (gx, max(lane_trips(len(scene.probs[i][3]["u"]), gx) for i in idx))
    print("\nforms (gx, most trips per lane):", forms)
    gxs = {f[0] for f in forms.values()}
    assert {1, 2, 4} <= gxs and max(gxs) >= 8, forms
    for name, (gx, trips) in forms.items():
        assert trips >= 2 or name == "ragged", (name, forms)                  # (the ragged batch is the fold's form: gx >= 8, one trip)
    assert forms["bench640"][0] == 4 and len(batches(scene, n_cu)["bench641"]) % 8 == 1
    # the ragged batch folds fewer partials than gx for its small problems (k_track_finalize: nb = min(gx, ceil(n / 256)))
    idx = batches(scene, n_cu)["ragged"]
    gx = forms["ragged"][0]
    assert any(max(1, -(-len(scene.probs[i][3]["u"]) // TRK_BLOCK)) < gx for i in idx)
    assert {len(scene.probs[i][3]["u"]) for i in idx} >= {0, 1, 255, 256, 257, 1024, 1025}


def test_per_point_terms_restated_in_f64(scene):
    """(2) the oracle's warped points (the truth's input) against a plain f64 calcRes: the same inliers, the same terms at float tolerance,
    except the few points whose bounds / cut-off decision sits within float noise of its threshold"""
    tot = edge = 0
    n_checked = 0
    for e in scene.exp:
        if "restated" in e:
            ed, n = e["restated"]
            edge += ed
            tot += n
            n_checked += 1
    assert n_checked >= 10 + 3 * len(SIZES) and tot > 100000
    assert edge <= 1e-3 * tot, (edge, tot)                   # measured: 59 of 174 201


def test_single_evaluations_against_truth(gpu_ctx, scene):
    """sdso_track_calc_res_gs (gx = ceil(n / 256), one trip) on every level of two frames and every template size; masks bit-exact"""
    st = Stats()
    idx = [i for i, p in enumerate(scene.probs) if p[1] in (0, 57) and i < scene.nbench] + [i for n in SIZES for i in scene.sub[n]]
    for i in idx:
        ref, f, lvl, pc_l, ev = scene.probs[i]
        n = len(pc_l["u"])
        H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0); mask = np.zeros(max(n, 1), np.uint8)
        gpu_ctx.check(gpu_ctx.L.sdso_track_calc_res_gs(gpu_ctx.h, ref, FRAME0 + f, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res),
                                                        C.byref(nw), abi.bp(mask)))
        assert np.array_equal(mask[:n], scene.exp[i]["mask"]), i
        check_problem(("single", i, n), H, b, res, nw.value, scene.exp[i], st)
    assert_not_noisier(st, "single")


@pytest.mark.parametrize("name", ["bench640", "bench641", "gx2", "gx1"])
def test_batched_against_truth(gpu_ctx, scene, n_cu, name):
    """(3) sdso_track_batch_prepare -> enqueue -> fetch, the benchmarked entry points, at the bench's shape and the forms around it"""
    idx = batches(scene, n_cu)[name]
    H, b, res, nw = run_batch(gpu_ctx, scene, idx)
    st = Stats()
    for k, i in enumerate(idx):
        check_problem((name, k, i), H[k], b[k], res[k], int(nw[k]), scene.exp[i], st)
    assert_not_noisier(st, name)


def test_ragged_batch_folds_only_its_partials(gpu_ctx, scene, n_cu):
    """n = 0, 1, 255, 256, 257, 1024, 1025 beside large templates in one launch (gx >= 8): the small problems' workgroups past their
    points exit early and k_track_finalize folds only the nb partials that were written.  A batch of the same count and largest template
    runs first, so every partial slot of the layout holds another problem's sums."""
    idx = batches(scene, n_cu)["ragged"]
    big = scene.sub[20000][:2]
    poison = [big[k % 2] for k in range(len(idx))]
    assert choose_gx(n_cu, len(poison), scene.maxn(poison)) == choose_gx(n_cu, len(idx), scene.maxn(idx))
    st = Stats()
    Hp, bp_, rp, nwp = run_batch(gpu_ctx, scene, poison)
    for k, i in enumerate(poison):
        check_problem(("poison", k), Hp[k], bp_[k], rp[k], int(nwp[k]), scene.exp[i], st)
    H, b, res, nw = run_batch(gpu_ctx, scene, idx)
    for k, i in enumerate(idx):
        e = scene.exp[i]
        check_problem(("ragged", k, len(scene.probs[i][3]["u"])), H[k], b[k], res[k], int(nw[k]), e, st)
        if e["nw"] == 0:
            assert not H[k].any() and not b[k].any()
    assert_not_noisier(st, "ragged")


def test_prepared_batch_lifecycle(oracle, scene):
    """the prepared batch as bench.py uses it, on a context of its own (its buffers start empty and grow): repeated enqueues, partial
    fetches, invalidation by a single evaluation, a later larger prepare"""
    ctx = abi.Context(0)
    try:
        L = ctx.L
        frames = (0, 57, 127)
        rs = np.random.RandomState(77)
        imgs = {}
        for f in range(NFRAMES):
            img = scene.frame_image(rs)
            if f in frames:
                imgs[f] = img
        for f in frames:
            ctx.check(L.sdso_make_pyramid(ctx.h, FRAME0 + f, W0, H0, abi.fp(imgs[f])))
        ctx.set_ref(REF0, scene.prob["pc"])
        for k, n in enumerate(SIZES):
            ctx.set_ref(REFSUB0 + k, [subset(scene.big["pc"][0], n)] + [EMPTY] * (scene.levels - 1))
        small = [i for i, p in enumerate(scene.probs) if p[1] == 0 and i < scene.nbench]                  # 5 problems
        large = [i for i, p in enumerate(scene.probs) if p[1] in frames] * 4                               # > cap and part_cap of `small`
        st = Stats()

        def fetch(n, want=(True, True, True, True), rows=None):
            rows = n + 3 if rows is None else rows
            H = np.full((rows, 64), -7.0); b = np.full((rows, 8), -7.0); res = np.full((rows, 6), -7.0); nw = np.full(rows, -7, np.int32)
            rc = L.sdso_track_batch_fetch(ctx.h, abi.dp(H) if want[0] else None, abi.dp(b) if want[1] else None,
                                          abi.dp(res) if want[2] else None, abi.ip(nw) if want[3] else None)
            return rc, H, b, res, nw

        def prepare(idx):
            refs, fr, evs = scene.slots(idx)
            ctx.check(L.sdso_track_batch_prepare(ctx.h, len(idx), abi.ip(refs), abi.ip(fr), evs))

        prepare(small)
        ctx.check(L.sdso_track_batch_enqueue(ctx.h))
        rc, H1, b1, r1, n1 = fetch(len(small))
        assert rc == 0
        ctx.check(L.sdso_track_batch_enqueue(ctx.h))                                                       # no new prepare
        rc, H2, b2, r2, n2 = fetch(len(small))
        assert rc == 0
        for x, y in ((H1, H2), (b1, b2), (r1, r2), (n1, n2)):
            assert np.array_equal(x, y, equal_nan=True)                                                    # bit-identical
            assert (x[len(small):] == -7).all()                                                            # nothing past nprob
        for k, i in enumerate(small):
            check_problem(("small", k), H1[k], b1[k], r1[k], int(n1[k]), scene.exp[i], st)
        # NULL outputs: only what was asked for is filled, and it is what the full fetch returned
        rc, H3, b3, r3, n3 = fetch(len(small), want=(True, False, False, True))
        assert rc == 0 and np.array_equal(H3, H1) and np.array_equal(n3, n1) and (b3 == -7).all() and (r3 == -7).all()
        rc, H3, b3, r3, n3 = fetch(len(small), want=(False, True, True, False))
        assert rc == 0 and np.array_equal(b3, b1) and np.array_equal(r3, r1, equal_nan=True) and (H3 == -7).all() and (n3 == -7).all()
        # a single evaluation between prepare and enqueue overwrites the batch's first problem record: the batch is gone
        prepare(small)
        ref, f, lvl, pc_l, ev = scene.probs[scene.sub[4097][0]]
        H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0)
        ctx.check(L.sdso_track_calc_res_gs(ctx.h, ref, FRAME0 + f, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res), C.byref(nw), None))
        check_problem("single between", H, b, res, nw.value, scene.exp[scene.sub[4097][0]], st)
        assert L.sdso_track_batch_enqueue(ctx.h) != 0
        rc, H4, b4, r4, n4 = fetch(len(small))
        assert rc != 0 and (H4 == -7).all() and (n4 == -7).all()
        # ... and after enqueue, before fetch, likewise: no stale results
        prepare(small)
        ctx.check(L.sdso_track_batch_enqueue(ctx.h))
        ctx.check(L.sdso_track_calc_res_gs(ctx.h, ref, FRAME0 + f, C.byref(ev), None, None, None, None, None))
        rc, H4, b4, r4, n4 = fetch(len(small))
        assert rc != 0 and (H4 == -7).all() and (n4 == -7).all()
        # a larger prepare grows the problem table and the partials: still the truth
        prepare(large)
        ctx.check(L.sdso_track_batch_enqueue(ctx.h))
        rc, H5, b5, r5, n5 = fetch(len(large))
        assert rc == 0
        for k, i in enumerate(large):
            check_problem(("large", k, i), H5[k], b5[k], r5[k], int(n5[k]), scene.exp[i], st)
        assert_not_noisier(st, "lifecycle")
    finally:
        ctx.close()


@pytest.mark.parametrize("G,n0", [(1, 12000), (8, 20000)])
def test_resident_lm_on_multi_trip_template(gpu_ctx, oracle, scene, n_cu, monkeypatch, G, n0):
    """(4) k_track_lm on a level-0 template of several trips per lane (one trip: LM_UNROLL * LM_BLOCK * G points; the first comes from
    registers, the later ones load their points): pose within 1e-5 and the iteration counts of the oracle's trackNewestCoarse (up to the
    oracle's own knife-edge decisions, see test_tracker_gpu.py::test_cluster_sizes_reproduce_the_iteration_counts), and the evaluation at
    the final pose against the truth"""
    big = scene.big
    pcs = [subset(big["pc"][0], n0)] + list(big["pc"][1:])
    prob = dict(big)
    prob["pc"] = pcs
    slot_ref, slot_new = 620 + G, 630 + G
    gpu_ctx.upload_pyramid(slot_new, big["pyr_new"])
    gpu_ctx.set_ref(slot_ref, pcs)
    slots8 = 8
    g_eff = min(LM_MAXG, (n_cu * 7 // 8) // slots8, G)       # the choice of G in sdso_track_newest_coarse_batch (tracker_lm_api.hip), for one hypothesis
    g_eff = 1 if g_eff < 2 else g_eff
    assert g_eff == G
    assert -(-n0 // (LM_UNROLL * LM_BLOCK * G)) >= 2 and -(-len(pcs[1]["u"]) // (LM_UNROLL * LM_BLOCK * G)) >= 2
    prm = helpers.track_params(prob)
    To, affo, outo = helpers.oracle_track(oracle, prob, prm, (np.eye(3), np.zeros(3)), (0.0, 0.0))
    m = np.zeros(5)
    oracle.orc_track_last_margins(abi.dp(m))
    monkeypatch.setenv("SDSO_TRK_LM_CLUSTER", str(G))
    T = abi.SE3.from_Rt(np.eye(3), np.zeros(3)); aff = abi.Aff(0, 0); out = abi.TrackResult()
    try:
        gpu_ctx.check(gpu_ctx.L.sdso_track_newest_coarse(gpu_ctx.h, slot_ref, slot_new, C.byref(prm), C.byref(T), C.byref(aff), C.byref(out)))
    finally:
        monkeypatch.delenv("SDSO_TRK_LM_CLUSTER")
    assert out.good == outo.good == 1
    R, t = T.Rt(); Ro, to = To.Rt()
    assert np.abs(t - to).max() <= 1e-5 and np.abs(R - Ro).max() <= 1e-5
    assert abs(aff.a - affo.a) <= 1e-5 and abs(aff.b - affo.b) <= 1e-3
    if list(out.iterations) != list(outo.iterations) or out.evaluations != outo.evaluations:
        lv = [l for l in range(5) if out.iterations[l] != outo.iterations[l]]
        assert lv and min(m[l] for l in range(max(lv), 5)) <= 1e-5, (list(out.iterations), list(outo.iterations), m)
    else:
        assert out.point_evals == outo.point_evals
    for l in range(prob["levels"]):
        assert abs(out.lastResiduals[l] - outo.lastResiduals[l]) <= 1e-4 * outo.lastResiduals[l]
    # every level's system at the pose the call ended on, device (calc_res_gs) against the truth
    st = Stats()
    for lvl in range(prob["levels"]):
        ev = abi.TrackEval()
        gpu_ctx.L.sdso_track_make_eval(C.byref(prm), lvl, C.byref(T), C.byref(aff), 1.0, C.byref(ev))
        Ho, bo, reso, nwo, masko, buf = helpers.oracle_eval_warped(oracle, pcs[lvl], big["pyr_new"][lvl], ev)
        exp = dict(H=Ho, b=bo, res=reso, nw=nwo, truth=truth(pcs[lvl], ev, reso, nwo, masko, buf))
        H = np.zeros(64); b = np.zeros(8); res = np.zeros(6); nw = C.c_int(0)
        gpu_ctx.check(gpu_ctx.L.sdso_track_calc_res_gs(gpu_ctx.h, slot_ref, slot_new, C.byref(ev), abi.dp(H), abi.dp(b), abi.dp(res), C.byref(nw), None))
        check_problem(("lm final", G, lvl), H, b, res, nw.value, exp, st)
    print("\nLM G=%d n0=%d: iterations %s / oracle %s; %r" % (G, n0, list(out.iterations), list(outo.iterations), st))
    gpu_ctx.L.sdso_track_release_ref(gpu_ctx.h, slot_ref)
    gpu_ctx.L.sdso_release_pyramid(gpu_ctx.h, slot_new)
