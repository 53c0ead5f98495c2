"""NumPy statement of the keyframe's published depth image, in float32 where the reference is float.

level0_map      idepth[0] as CoarseTracker::makeCoarseDepthL0 leaves it (CoarseTracker.cpp:352-354 STEP1's ordered +=, :390-441 STEP3 at
                level 0, :492-533 STEP5 at level 0; level 0 does not depend on the other levels): inside [2,w-2) x [2,h-2) the normalised
                inverse depth or -1, in the two-pixel border the un-normalised sums STEP1 and STEP3 left.
select_range    :1078-1088 with the sort
smooth_range    :1094-1117
draw            :1119-1163 as the literal loops, setPixelCirc's scatter in raster order included
debug_plot      the whole of debugPlotIDepthMap, with the library's stated deviation for a map without a positive pixel

The reference's x86 build converts a NaN to INT_MIN: makeJet3B then matches no case and returns white, the background byte is 0."""
import numpy as np

f32 = np.float32


def random_points(w, h, n, seed):
    """n points uniform over the WHOLE image (rows and columns 0, 1, w-2, w-1 included), idepth U(0.05, 2), weight U(0.1, 30)"""
    rs = np.random.RandomState(seed)
    u = rs.randint(0, w, n).astype(np.int32)
    v = rs.randint(0, h, n).astype(np.int32)
    return u, v, rs.uniform(0.05, 2.0, n).astype(f32), rs.uniform(0.1, 30.0, n).astype(f32)


def level0_map(u, v, new_idepth, weight, I0):
    """I0: the level-0 intensities [h, w] of lastRef (STEP5 drops a pixel whose colour is not finite)"""
    h, w = I0.shape
    idl = np.zeros(w * h, f32)
    wsl = np.zeros(w * h, f32)
    for i in range(len(u)):                                   # STEP1: in point order
        k = int(u[i]) + w * int(v[i])
        idl[k] = idl[k] + f32(new_idepth[i]) * f32(weight[i])
        wsl[k] = wsl[k] + f32(weight[i])
    bak = wsl.copy()                                          # STEP3: reads where bak > 0, writes where bak <= 0
    src = idl.copy()
    idx = np.arange(w, w * h - w)
    s = np.zeros(len(idx), f32); num = np.zeros(len(idx), f32); numn = np.zeros(len(idx), f32)
    for o in (1 + w, -1 - w, w - 1, -w + 1):
        j = idx + o
        inside = (j >= 0) & (j < w * h)                                    # (the reference reads one element past the map at the last pixel; skipped)
        jj = np.where(inside, j, 0)
        ok = inside & (bak[jj] > 0)
        s = np.where(ok, s + src[jj], s).astype(f32)
        num = np.where(ok, num + bak[jj], num).astype(f32)
        numn = np.where(ok, numn + f32(1), numn).astype(f32)
    upd = (bak[idx] <= 0) & (numn > 0)
    idl[idx[upd]] = (s[upd] / numn[upd]).astype(f32)
    wsl[idx[upd]] = (num[upd] / numn[upd]).astype(f32)
    m = idl.reshape(h, w)                                     # STEP5 on [2,w-2) x [2,h-2)
    ws = wsl.reshape(h, w)[2:h - 2, 2:w - 2]
    inner = m[2:h - 2, 2:w - 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (inner / ws).astype(f32)
    keep = (ws > 0) & np.isfinite(I0[2:h - 2, 2:w - 2]) & (q > 0)
    m[2:h - 2, 2:w - 2] = np.where(keep, q, f32(-1))
    return m


def select_range(m):
    """-> (minID_new, maxID_new, allID.size()); the two values are None for an empty allID"""
    allID = np.sort(m.reshape(-1)[m.reshape(-1) > 0])
    if len(allID) == 0:
        return None, None, 0
    n = len(allID) - 1
    return allID[int(n * 0.05)], allID[int(n * 0.95)], len(allID)


def smooth_range(minID, maxID, prev):
    """prev = (*minID_pt, *maxID_pt) or None -> the range the image is drawn with (and, with prev, what the two values become)"""
    minID, maxID = f32(minID), f32(maxID)
    if prev is None:
        return minID, maxID
    p0, p1 = f32(prev[0]), f32(prev[1])
    if p0 < 0 or p1 < 0:
        return minID, maxID
    maxChange = f32(0.3 * float(f32(p1 - p0)))
    if minID < f32(p0 - maxChange): minID = f32(p0 - maxChange)
    if minID > f32(p0 + maxChange): minID = f32(p0 + maxChange)
    if maxID < f32(p1 - maxChange): maxID = f32(p1 - maxChange)
    if maxID > f32(p1 + maxChange): maxID = f32(p1 + maxChange)
    return minID, maxID


def background(I0):
    with np.errstate(invalid="ignore"):
        p = (I0.astype(f32) * f32(0.9)).astype(f32)
        ok = np.isfinite(p) & (np.abs(p) < 2.0 ** 31)
        c = np.where(ok, np.trunc(np.where(ok, p, 0)), -2.0 ** 31).astype(np.int64)
    c = np.where(c > 255, 255, c)
    return (c & 0xFF).astype(np.uint8)


def make_jet_3b(id_):
    """makeJet3B (globalFuncs.h:362-379) on a float32 array -> ([n, 3] uint8, the outcome per entry: -1 / 8 the two clamps, 0..7 icP, 9 NaN)"""
    id_ = np.asarray(id_, f32)
    n = len(id_)
    out = np.full((n, 3), 255, np.uint8)
    case = np.full(n, 9, np.int32)
    nan = np.isnan(id_)
    with np.errstate(invalid="ignore"):
        lo = ~nan & (id_ <= 0)
        hi = ~nan & ~lo & (id_ >= 1)
    out[lo] = (128, 0, 0); case[lo] = -1
    out[hi] = (0, 0, 128); case[hi] = 8
    mid = ~nan & ~lo & ~hi
    t = (id_[mid] * f32(8)).astype(f32)
    icP = np.trunc(t).astype(np.int32)
    ifP = (t - icP.astype(f32)).astype(f32).astype(np.float64)
    z = np.zeros(len(t))
    full = np.full(len(t), 255.0)
    chans = {0: (255 * (0.5 + 0.5 * ifP), z, z), 1: (full, 255 * (0.5 * ifP), z), 2: (full, 255 * (0.5 + 0.5 * ifP), z),
             3: (255 * (1 - 0.5 * ifP), full, 255 * (0.5 * ifP)), 4: (255 * (0.5 - 0.5 * ifP), full, 255 * (0.5 + 0.5 * ifP)),
             5: (z, 255 * (1 - 0.5 * ifP), full), 6: (z, 255 * (0.5 - 0.5 * ifP), full), 7: (z, z, 255 * (1 - 0.5 * ifP))}
    col = np.full((len(t), 3), 255, np.uint8)
    for k, ch in chans.items():
        sel = icP == k
        for c in range(3):
            col[sel, c] = np.trunc(ch[c][sel]).astype(np.uint8)
    out[mid] = col
    case[mid] = icP
    return out, case


RING = np.array([[abs(dx) >= 2 or abs(dy) >= 2 for dx in range(-3, 4)] for dy in range(-3, 4)])   # setPixelCirc's 40 pixels


def draw(m, I0, minID, maxID, overlay=True):
    """-> dict(rgb [h, w, 3], circles, case per source, centre_positive per source, sources (y, x))"""
    h, w = m.shape
    bg = background(I0)
    rgb = np.repeat(bg[:, :, None], 3, axis=2).copy()
    if not overlay:
        return dict(rgb=rgb, circles=0, case=np.zeros(0, np.int32), centre_positive=np.zeros(0, bool), sources=(np.zeros(0, int), np.zeros(0, int)))
    taps = [m[3:h - 3, 3:w - 3], m[3:h - 3, 4:w - 2], m[3:h - 3, 2:w - 4], m[4:h - 2, 3:w - 3], m[2:h - 4, 3:w - 3]]   # bp[0], bp[1], bp[-1], bp[wl], bp[-wl]
    sid = np.zeros(taps[0].shape, f32)
    nid = np.zeros(taps[0].shape, f32)
    for t in taps:
        pos = t > 0
        sid = np.where(pos, sid + t, sid).astype(f32)
        nid = np.where(pos, nid + f32(1), nid).astype(f32)
    qual = (taps[0] > 0) | (nid >= 3)
    ys, xs = np.nonzero(qual)                                 # raster order
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        id_ = ((((sid[ys, xs] / nid[ys, xs]).astype(f32) - f32(minID)).astype(f32)) / f32(f32(maxID) - f32(minID))).astype(f32)
    col, case = make_jet_3b(id_)
    ys, xs = ys + 3, xs + 3
    for k in range(len(ys)):                                  # the scatter: later sources overwrite earlier ones
        rgb[ys[k] - 3:ys[k] + 4, xs[k] - 3:xs[k] + 4][RING] = col[k]
    return dict(rgb=rgb, circles=len(ys), case=case, centre_positive=(taps[0] > 0)[ys - 3, xs - 3], sources=(ys, xs))


def debug_plot(m, I0, prev=None):
    """debugPlotIDepthMap -> dict(rgb, counts (allID.size(), circles), used (minID, maxID), prev_out (what *minID_pt, *maxID_pt hold after
    the call; prev itself for an empty map), new (minID_new, maxID_new), and draw's per-source records)"""
    lo, hi, count = select_range(m)
    if count == 0:
        d = draw(m, I0, 0, 0, overlay=False)
        d.update(counts=(0, 0), used=None, prev_out=prev, new=None)
        return d
    used = smooth_range(lo, hi, prev)
    d = draw(m, I0, used[0], used[1])
    d.update(counts=(count, d["circles"]), used=used, prev_out=used if prev is not None else None, new=(lo, hi))
    return d


# ------------------------------------------------------------------ the cases of tests/test_depth_image_*.py, stated once
SHAPES = {"96x64": (96, 64, 300, 9601), "322x242": (322, 242, 3000, 32201), "640x480": (640, 480, 20000, 64001)}   # w, h, points, seed
_cases = {}


def case(name):
    """-> dict(w, h, pyr (the frame's pyramid), I0, points (u, v, idepth, weight), map, plot = debug_plot(map, I0, (-1, -1))); computed once
    and shared: treat it as read-only"""
    if name not in _cases:
        import synth
        w, h, n, seed = SHAPES[name]
        pyr = synth.tracker_problem(w=w, h=h, npts=40, seed=seed)["pyr_ref"]
        I0 = np.ascontiguousarray(pyr[0][..., 0])
        pts = random_points(w, h, n, seed)
        m = level0_map(*pts, I0)
        _cases[name] = dict(w=w, h=h, pyr=pyr, I0=I0, points=pts, map=m, plot=debug_plot(m, I0, (f32(-1), f32(-1))))
    return _cases[name]


def border_mask(w, h):
    b = np.ones((h, w), bool)
    b[2:h - 2, 2:w - 2] = False
    return b


def input_conditions(name):
    """what the issue demands of the inputs -> dict of the figures the tests assert on"""
    c = case(name)
    p = c["plot"]
    return dict(outcomes=sorted(set(p["case"].tolist())), circles_without_centre=int((~p["centre_positive"]).sum()),
                border_positive=int((c["map"][border_mask(c["w"], c["h"])] > 0).sum()), positive=p["counts"][0], circles=p["counts"][1],
                levels=len(c["pyr"]))
