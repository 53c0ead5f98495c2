"""CPU checks of the immature-point set: the host-only removal order of the library against the reference's loop, and the conditions
that keep tests/test_immature_gpu.py from passing vacuously, on the CPU statement alone."""
import numpy as np
import pytest

from sdso_amd import abi
import immature_cases as Cs
import immature_ref as R


def _lib_order(flags):
    L = abi.load()
    flags = np.ascontiguousarray(flags, np.uint8)
    n = len(flags)
    src = np.full(max(n, 1), -7, np.int32)
    n_out = np.zeros(1, np.int32)
    assert L.sdso_imm_remove_order(n, abi.bp(flags), abi.ip(n_out), abi.ip(src)) == 0
    return list(src[:n_out[0]])


def _masks():
    rs = np.random.RandomState(77)
    yield "all", np.ones(37, np.uint8)
    yield "none", np.zeros(37, np.uint8)
    last = np.zeros(37, np.uint8); last[-1] = 1
    yield "last", last
    run = np.zeros(37, np.uint8); run[-9:] = 1; run[3] = 1; run[20] = 1
    yield "run at the back", run
    yield "alternating", (np.arange(38) % 2).astype(np.uint8)
    yield "alternating, last kept", (np.arange(37) % 2).astype(np.uint8)
    yield "n = 0", np.zeros(0, np.uint8)
    yield "n = 1 kept", np.zeros(1, np.uint8)
    yield "n = 1 flagged", np.ones(1, np.uint8)
    for k in range(200):
        n = int(rs.randint(1, 300))
        yield "random %d" % k, (rs.rand(n) < rs.choice([0.05, 0.5, 0.95])).astype(np.uint8)


def test_remove_order_is_the_reference_loop():
    for name, flags in _masks():
        want = R.remove_order(list(flags))
        assert _lib_order(flags) == want, name
        assert sorted(want) == [i for i in range(len(flags)) if not flags[i]], name      # exactly the unflagged entries survive
    L = abi.load()
    assert L.sdso_imm_remove_order(-1, None, abi.ip(np.zeros(1, np.int32)), None) == -1
    assert L.sdso_imm_remove_order(3, None, abi.ip(np.zeros(1, np.int32)), None) == -1


@pytest.fixture(scope="module")
def case():
    return Cs.window_case()


def test_case_covers_every_branch(oracle, case):
    """Three non-key frames on the large host alone (the statement, no device): every
    traceOn status and every forward traceStereo status occurs, the stereo rule rejects points, intervals are updated by the hundred,
    and no point is unreadable."""
    S = R.add_frame(oracle, case["hosts"][0]["img"], case["hosts"][0]["map"])
    assert len(S["u"]) == Cs.HOST_POINTS[0]
    on, fwd, tot = np.zeros(6, np.int64), np.zeros(6, np.int64), np.zeros(abi.IMM_NCOUNTS, np.int64)
    for k in range(3):
        F = case["frames"][k]
        counts, on_hist, fwd_hist = R.trace(oracle, [(S, F["geom"][0])], F["left"], F["right"], case["K4"], case["Ki"], case["baseline"])
        print("frame", k + 1, "traceOn", on_hist[:5], "forward", fwd_hist[:5], "stereo outliers", counts[R.C_STEREO_OUTLIER], "updated", counts[R.C_UPDATED],
              "unreadable", counts[R.C_UNREADABLE])
        assert on_hist.sum() == Cs.HOST_POINTS[0] and counts[:6].sum() == Cs.HOST_POINTS[0]
        assert counts[R.GOOD] == on_hist[R.GOOD] - counts[R.C_STEREO_OUTLIER]
        on += on_hist; fwd += fwd_hist; tot += counts
    assert (on[:5] > 0).all() and on[R.UNINITIALIZED] == 0
    assert (fwd[:5] > 0).all()
    assert tot[R.C_STEREO_OUTLIER] >= 1 and tot[R.C_UPDATED] >= 100 and tot[R.C_UNREADABLE] == 0


def test_crafted_map_drops_and_borders(oracle):
    """The statement on the crafted map: border entries are not candidates, the pixels just inside are, and some candidates are dropped
    for a non-finite energyTH.  A guard on the case and the statement only: it does not touch the library, so unlike the other new tests
    it also passes on a tree without sdso_imm_*; tests/test_immature_gpu.py compares the device with this statement on this case."""
    c = Cs.crafted_map_case()
    S = R.add_frame(oracle, c["img"], c["map"])
    inner = c["map"][3:Cs.H - 4, 3:Cs.W - 4]
    ncand = int((inner != 0).sum())
    assert int((c["map"] != 0).sum()) == ncand + 9
    assert 0 < ncand - len(S["u"]) <= 40
    pts = set(zip(S["u"].astype(int), S["v"].astype(int)))
    assert {(3, 240), (Cs.W - 5, 241), (320, 3), (321, Cs.H - 5)} <= pts
    assert set(np.unique(S["my_type"])) == {1.0, 2.0, 4.0}
    order = S["v"].astype(np.int64) * Cs.W + S["u"].astype(np.int64)
    assert (np.diff(order) > 0).all()                                                 # raster order
    assert np.isfinite(S["color"]).all() and (S["energyTH"] == 8 * 144).all()
