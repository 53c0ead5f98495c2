"""CPU statement of CoarseDistanceMap and of the candidate selection of FullSystem::activatePointsMT, for the tests.

Written from the behaviour of the reference (paths under src/FullSystem):
  CoarseDistanceMap::makeDistanceMap   CoarseTracker.cpp:1216-1255
  CoarseDistanceMap::growDistBFS       CoarseTracker.cpp:1260-1363   (list-ordered: bfsList1 / bfsList2, k = 1..39)
  CoarseDistanceMap::addIntoDistFinal  CoarseTracker.cpp:1366-1372
  FullSystem::activatePointsMT STEP 1  FullSystem.cpp:798-817        (currentMinActDist)
  FullSystem::activatePointsMT STEP 2  FullSystem.cpp:837-902        (delete / keep / select, re-growth after every selection)
Arithmetic is NumPy float32, one rounding per operation, products summed left to right (the convention of oracle/orc_math.h:33-42).
The map is a flat Python list of ints (0..39, FAR = 1000) while it is worked on; the public functions return float32 arrays.
"""
import numpy as np

FAR = 1000
KEEP, DELETE, SELECT = 0, 1, 2
IPS_GOOD, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED = range(6)     # ImmaturePoint.h:50-56

# neighbour order of growDistBFS: right, left, below, above (:1284-1306), then the four corners (:1341-1359)
_N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
_N8 = _N4 + ((1, 1), (-1, 1), (-1, -1), (1, -1))

f32 = np.float32


def project(KRKi, Kt, pg, u, v, idepth, w1, h1):
    """ptp = KRKi * (u, v, 1) + Kt * idepth, iu = int(ptp[0] / ptp[2] + 0.5f), iv likewise (CoarseTracker.cpp:1242-1246,
    FullSystem.cpp:883-887).  Returns (inside, iu, iv, ptp0); a quotient that is not finite or does not fit an int is outside."""
    A = np.asarray(KRKi, f32).reshape(-1, 9)[pg]
    t = np.asarray(Kt, f32).reshape(-1, 3)[pg]
    u, v, idepth = np.asarray(u, f32), np.asarray(v, f32), np.asarray(idepth, f32)
    one = f32(1)
    with np.errstate(all="ignore"):
        p = [((A[:, 3 * r] * u + A[:, 3 * r + 1] * v) + A[:, 3 * r + 2] * one) + t[:, r] * idepth for r in range(3)]
        qx = p[0] / p[2] + f32(0.5)
        qy = p[1] / p[2] + f32(0.5)
    ok = np.isfinite(qx) & np.isfinite(qy) & (np.abs(qx) < 2.0e9) & (np.abs(qy) < 2.0e9)
    iu = np.where(ok, qx, 0).astype(np.int64)        # float -> int truncates toward zero, like the C conversion
    iv = np.where(ok, qy, 0).astype(np.int64)
    inside = ok & (iu > 0) & (iv > 0) & (iu < w1) & (iv < h1)
    return inside, iu.astype(np.int32), iv.astype(np.int32), p[0].astype(f32)


def grow_bfs(m, w1, h1, lst):
    """growDistBFS on the flat list `m`, starting from the pixel list `lst` (the seeds are already 0 in m)."""
    for k in range(1, 40):
        cur, lst = lst, []
        nb = _N4 if k % 2 == 0 else _N8
        for (x, y) in cur:
            if x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1:       # :1279
                continue
            idx = x + y * w1
            for dx, dy in nb:
                j = idx + dx + dy * w1
                if m[j] > k:
                    m[j] = k
                    lst.append((x + dx, y + dy))
        if not lst:
            break


def make_list(w1, h1, seeds):
    """makeDistanceMap from the seed pixels [(iu, iv), ...] in list order -> flat list."""
    m = [FAR] * (w1 * h1)
    for (x, y) in seeds:
        m[x + w1 * y] = 0
    grow_bfs(m, w1, h1, list(seeds))
    return m


def add_into(m, w1, h1, u, v):
    """addIntoDistFinal(u, v): only pixels newly set by this call propagate."""
    m[u + w1 * v] = 0
    grow_bfs(m, w1, h1, [(u, v)])


def make_distance_map(w, h, KRKi, Kt, pg, u, v, idepth):
    """-> (map float32 (h1, w1), n_seeds, flat list for further work)"""
    w1, h1 = w >> 1, h >> 1
    if len(u):
        inside, iu, iv, _ = project(KRKi, Kt, np.asarray(pg), u, v, idepth, w1, h1)
        seeds = [(int(x), int(y)) for x, y in zip(iu[inside], iv[inside])]
    else:
        seeds = []
    m = make_list(w1, h1, seeds)
    return np.array(m, f32).reshape(h1, w1), len(seeds), m


def make_stencil(w1, h1, seeds):
    """The level-synchronous restatement: a pixel becomes k iff it is unassigned and a neighbour in N(k) that is not on the outer
    border holds exactly k-1."""
    m = np.full((h1, w1), FAR, np.int32)
    for (x, y) in seeds:
        m[y, x] = 0
    interior = np.zeros((h1, w1), bool)
    interior[1:-1, 1:-1] = True
    for k in range(1, 40):
        src = (m == k - 1) & interior
        hit = np.zeros((h1, w1), bool)
        for dx, dy in (_N4 if k % 2 == 0 else _N8):
            # pixel (x, y) has the neighbour (x - dx, y - dy) = src shifted by (dx, dy)
            sh = np.zeros((h1, w1), bool)
            ys, yd = (slice(0, h1 - dy), slice(dy, h1)) if dy >= 0 else (slice(-dy, h1), slice(0, h1 + dy))
            xs, xd = (slice(0, w1 - dx), slice(dx, w1)) if dx >= 0 else (slice(-dx, w1), slice(0, w1 + dx))
            sh[yd, xd] = src[ys, xs]
            hit |= sh
        m[hit & (m == FAR)] = k
    return m.astype(f32)


def closed_form_single_seed(w1, h1, sx, sy):
    """A single interior seed far from the border: the smallest k <= 39 with max(|dx|,|dy|) <= k and
    |dx|+|dy| <= 2*ceil(k/2) + floor(k/2) (ceil(k/2) diagonal-capable and floor(k/2) axis-only steps among the first k), else 1000."""
    m = np.full((h1, w1), FAR, f32)
    for y in range(h1):
        for x in range(w1):
            dx, dy = abs(x - sx), abs(y - sy)
            for k in range(0, 40):
                if max(dx, dy) <= k and dx + dy <= 2 * ((k + 1) // 2) + k // 2:
                    m[y, x] = k
                    break
    return m


def update_min_act_dist(current, n_points, desired=2000.0):
    """STEP 1 (FullSystem.cpp:798-817): `float currentMinActDist` updated with double literals; the thresholds are
    float * double products compared with the int ef->nPoints."""
    c = f32(current)
    d = np.float64(f32(desired))
    n = int(n_points)

    def sub(c, x):
        return f32(np.float64(c) - x)

    if n < d * 0.66:
        c = sub(c, 0.8)
    if n < d * 0.8:
        c = sub(c, 0.5)
    elif n < d * 0.9:
        c = sub(c, 0.2)
    elif n < d:
        c = sub(c, 0.1)
    if n > d * 1.5:
        c = sub(c, -0.8)
    if n > d * 1.3:
        c = sub(c, -0.5)
    if n > d * 1.15:
        c = sub(c, -0.2)
    if n > d:
        c = sub(c, -0.1)
    if c < 0:
        c = f32(0)
    if c > 4:
        c = f32(4)
    return c


def select(m, w, h, KRKi, Kt, flagged, pg, u, v, idepth_min, idepth_max, quality, interval, status, my_type, min_act_dist,
           min_trace_quality=3.0, regrow=True):
    """STEP 2 over the flattened candidates, in order, on the flat list `m` (updated in place when regrow).
    -> dict(decision uint8, iu, iv int32, reached bool (got as far as the distance test), n_selected, row (which rule decided))
    row: 0 DELETE by :850, 1 KEEP and 2 DELETE by :869-880, 3 DELETE by projection :897-900, 4 SELECT, 5 KEEP by distance."""
    w1, h1 = w >> 1, h >> 1
    n = len(u)
    pg = np.asarray(pg)
    imin, imax = np.asarray(idepth_min, f32), np.asarray(idepth_max, f32)
    status = np.asarray(status)
    with np.errstate(all="ignore"):
        mid = f32(0.5) * (imax + imin)
        inside, iu, iv, p0 = project(KRKi, Kt, pg, u, v, mid, w1, h1)
        frac = (p0 - np.floor(p0)).astype(f32)
        thr = (f32(min_act_dist) * np.asarray(my_type, f32)).astype(f32)
        can = (np.isin(status, (IPS_GOOD, IPS_SKIPPED, IPS_BADCONDITION, IPS_OOB)) & (np.asarray(interval, f32) < 8)
               & (np.asarray(quality, f32) > f32(min_trace_quality)) & ((imax + imin) > 0))
    dead = ~np.isfinite(imax) | (status == IPS_OUTLIER)
    dec = np.zeros(n, np.uint8)
    row = np.zeros(n, np.int8)
    reached = np.zeros(n, bool)
    nsel = 0
    flagged = np.asarray(flagged)
    for i in range(n):
        if dead[i]:
            dec[i], row[i] = DELETE, 0
        elif not can[i]:
            if flagged[pg[i]] or status[i] == IPS_OOB:
                dec[i], row[i] = DELETE, 2
            else:
                dec[i], row[i] = KEEP, 1
        elif not inside[i]:
            dec[i], row[i] = DELETE, 3
        else:
            reached[i] = True
            x, y = int(iu[i]), int(iv[i])
            dist = f32(m[x + w1 * y]) + frac[i]
            if dist >= thr[i]:
                if regrow:
                    add_into(m, w1, h1, x, y)
                dec[i], row[i] = SELECT, 4
                nsel += 1
            else:
                dec[i], row[i] = KEEP, 5
    return dict(decision=dec, iu=iu, iv=iv, reached=reached, n_selected=nsel, row=row)
