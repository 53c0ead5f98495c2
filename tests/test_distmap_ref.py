"""tests/distmap_ref.py — the CPU statement of CoarseDistanceMap::growDistBFS / addIntoDistFinal and of activatePointsMT STEP 1 —
pinned against values derived by hand, not against itself (no GPU)."""
import os
import subprocess

import numpy as np

import distmap_ref as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo-dso-g2o_amd", "host")


def _single(w1=100, h1=100, sx=50, sy=50):
    return np.array(R.make_list(w1, h1, [(sx, sy)]), np.float32).reshape(h1, w1)


def test_single_seed_first_rings_literal():
    """The alternating 8/4 metric: step 1 takes the 8 neighbours, step 2 only the 4-neighbours of those, ...  Worked by hand for the
    quadrant dx, dy = 0..5 (the map is symmetric in both axes)."""
    m = _single()
    q = m[50:56, 50:56].astype(int)
    expect = np.array([[0, 1, 2, 3, 4, 5],
                       [1, 1, 2, 3, 4, 5],
                       [2, 2, 3, 3, 4, 5],
                       [3, 3, 3, 4, 5, 5],
                       [4, 4, 4, 5, 5, 6],
                       [5, 5, 5, 5, 6, 7]])
    assert np.array_equal(q, expect)
    assert list(q[2]) == [2, 2, 3, 3, 4, 5] and list(q[5]) == [5, 5, 5, 5, 6, 7]
    for flip in (m[50:56, 50:44:-1], m[50:44:-1, 50:56], m[50:44:-1, 50:44:-1]):
        assert np.array_equal(flip.astype(int), expect)


def test_single_seed_closed_form_everywhere():
    """Every pixel: the smallest k <= 39 with max(|dx|,|dy|) <= k and |dx|+|dy| <= 2*ceil(k/2) + floor(k/2), else 1000."""
    m = _single()
    cf = R.closed_form_single_seed(100, 100, 50, 50)
    assert np.array_equal(m, cf)
    assert m.max() == 1000 and (m == 39).any() and m[50, 50 + 39] == 39 and m[50, 50 + 40] == 1000


def test_border_seed_does_not_propagate():
    m = _single(sx=99, sy=50)
    assert m[50, 99] == 0 and (m != 1000).sum() == 1                    # the last column never propagates (x == w1-1)
    m = _single(sx=50, sy=99)
    assert m[99, 50] == 0 and (m != 1000).sum() == 1
    m = _single(sx=98, sy=50)                                           # one pixel inside: it does, also ONTO the border column ...
    assert m[50, 98] == 0 and m[50, 99] == 1 and m[49, 99] == 1 and m[51, 99] == 1 and m[50, 97] == 1
    # ... but what it set on the border does not carry on: (99, 52) is reached from (98, 51) at step 2? no — step 2 is axis-only,
    # (98, 51) -> (98, 52) at 2 -> (99, 52) is a diagonal/axis neighbour at step 3 (8-neighbourhood): 3, not 2 via the border column
    assert m[52, 99] == 3 and m[52, 98] == 2


def test_stencil_form_equals_list_form():
    rs = np.random.RandomState(3)
    for (w1, h1, n) in ((308, 92, 50), (308, 92, 600), (97, 61, 5)):
        seeds = [(int(x), int(y)) for x, y in zip(rs.randint(0, w1, n), rs.randint(0, h1, n))]
        a = np.array(R.make_list(w1, h1, seeds), np.float32).reshape(h1, w1)
        assert np.array_equal(a, R.make_stencil(w1, h1, seeds))


def test_add_into_only_new_pixels_propagate():
    """addIntoDistFinal lowers the map around the new seed and never raises it; where the map was already <= k the growth stops."""
    m = R.make_list(100, 100, [(30, 50)])
    before = np.array(m).reshape(100, 100)
    R.add_into(m, 100, 100, 40, 50)
    after = np.array(m).reshape(100, 100)
    assert (after <= before).all() and after[50, 40] == 0 and after[50, 41] == 1 and after[50, 30] == 0
    alone = np.array(R.make_list(100, 100, [(40, 50)])).reshape(100, 100)
    assert np.array_equal(after[50, 36:46], np.minimum(before, alone)[50, 36:46])
    assert np.array_equal(after[50, :31], before[50, :31])              # left of the old seed nothing changes


def test_min_act_dist_update_matches_shim():
    """STEP 1 at the eight thresholds (0.66, 0.8, 0.9, 1, 1, 1.15, 1.3, 1.5 times setting_desiredPointDensity), one point below, on
    and above each: the shim's float / double-literal arithmetic against the restatement, bit for bit; and the values by hand."""
    r = subprocess.run(["make", "-s", "-C", HOST, "test_distmap_shim"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(HOST, "test_distmap_shim")
    for desired in (2000.0, 4000.0):
        ns = sorted({int(desired * f) + d for f in (0.66, 0.8, 0.9, 1.0, 1.15, 1.3, 1.5) for d in (-1, 0, 1)})
        for cur in (2.0, 0.3, 3.9):
            out = subprocess.run([exe, "minact", repr(cur), repr(desired)] + [str(n) for n in ns], capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stderr
            got = np.array([float(x) for x in out.stdout.split()], np.float32)
            exp = np.array([R.update_min_act_dist(cur, n, desired) for n in ns], np.float32)
            assert np.array_equal(got, exp), (desired, cur)
    f = np.float32
    assert R.update_min_act_dist(2.0, 1319) == f(np.float64(f(np.float64(f(2.0)) - 0.8)) - 0.5)     # both `if`s fire below 0.66
    assert R.update_min_act_dist(2.0, 1320) == f(1.5) and R.update_min_act_dist(2.0, 1600) == f(np.float64(f(2.0)) - 0.2)
    assert R.update_min_act_dist(2.0, 2000) == f(2.0) and R.update_min_act_dist(2.0, 2001) == f(np.float64(f(2.0)) + 0.1)
    assert R.update_min_act_dist(0.3, 100) == 0 and R.update_min_act_dist(3.9, 10000) == 4             # the clamps
