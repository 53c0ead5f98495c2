"""CPU checks behind tests/test_marg_prior_gpu.py, on the oracle alone: the float oracle's own distance from the f64-accumulator truth on
HM / bM (the figure every device bar is derived from), and the conditions that keep the device comparisons from passing vacuously.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import marg_prior_cases as MP


@pytest.fixture(scope="module")
def table(oracle):
    return {(c, p): MP.reference(oracle, c, p) for c in MP.CASES for p in MP.PATTERNS}


def test_float_oracle_is_close_to_the_truth_on_every_case(oracle, table):
    """The non-vacuity condition: the bars of the device tests are 2 * E_H and 2 * E_b, and they can never silently widen.
    Measured: E_H 4.0e-6 (nf2_two_chunks / host0; 2.4e-6 without that window), E_b 1.1e-6 (nf2_two_chunks / all)."""
    for (c, p), (f32, f64) in table.items():
        print("%-16s %-7s e_H %.2e e_b %.2e" % (c, p, f32["e_H"], f32["e_b"]))
    E_H, E_b = MP.bars(oracle)
    print("E_H %.3e E_b %.3e" % (E_H, E_b))
    assert E_H <= 1e-5 and E_b <= 2e-6
    assert E_H == max(v[0]["e_H"] for v in table.values()) and E_b == max(v[0]["e_b"] for v in table.values())


def test_the_truth_mode_reaches_the_marginalisation(table):
    """orc_set_acc64 changes what orc_ba_marginalize_points returns wherever a point is flagged"""
    for (c, p), (f32, f64) in table.items():
        if p != "none":
            assert f32["e_H"] > 0, (c, p)
            assert f32["resInM"] == f64["resInM"] > 0, (c, p)
            assert np.array_equal(f32["state"], f64["state"]) and np.array_equal(f32["act"], f64["act"]) and np.array_equal(f32["jp"], f64["jp"])


@pytest.mark.parametrize("case", MP.CASES)
def test_case_has_the_shape_it_was_built_for(table, case):
    win = MP.window(case)
    n = 8 * win["nf"] + 4
    HM0, bM0 = MP.prior_in(win)
    for p in MP.PATTERNS:
        f32, f64 = table[(case, p)]
        flag = MP.flags(win, p)
        live = MP.live_of(f64["HM"])
        print(case, p, "flagged", int(flag.sum()), "of", win["np"], "resInM", f64["resInM"], "live", int(live.sum()), "of", n)
        if p == "none":
            assert not flag.any() and f64["resInM"] == 0
            assert np.array_equal(f64["HM"], HM0) and np.array_equal(f32["HM"], HM0)       # HM += 0.25 * (0 - 0): the prior, bit for bit
        else:
            assert 0 < flag.sum() and f64["resInM"] >= 1
            assert np.abs(f64["HM"] - HM0).max() > 0
        if p == "one":
            assert flag.sum() == 1 and MP.active_counts(win)[np.nonzero(flag)[0][0]] >= min(2, win["nf"] - 1)
            assert f64["resInM"] >= min(2, win["nf"] - 1)
        if p == "rand10":
            assert flag.sum() < win["np"] and (flag & (1 - MP.flags(win, "host0"))).any()
        if p in ("host0", "all"):
            assert live.sum() == n
        assert np.array_equal(f32["HM"] == 0, f64["HM"] == 0)
    if case == "nf2_two_chunks":
        print("largest (host, target) pair:", MP.largest_pair(win), "residuals of", win["nr"], "; points", win["np"])
        assert MP.largest_pair(win) > MP.CHUNK
        assert (win["np"], win["nr"]) == (600, 568)
    if case == "nf4_no_frame0":
        assert 0 not in win["frameID"]
    else:
        assert win["frameID"][0] == 0
    if case == "nf4_prior":
        assert np.abs(HM0).max() > 0 and np.abs(bM0).max() > 0
    else:
        assert not HM0.any() and not bM0.any()


def test_dead_points_window_has_flagged_points_of_every_kind(table):
    win = MP.window("nf4_dead_points")
    cnt = MP.residual_counts(win)
    outlier = np.zeros(win["np"], bool)
    outlier[win["res_point"][win["res_state"] == 2]] = True
    print("points", win["np"], "without residuals", int((cnt == 0).sum()), "with an OUTLIER residual", int(outlier.sum()),
          "hosted per frame", np.bincount(win["host"], minlength=win["nf"]).tolist())
    assert not (win["host"] == 1).any() and (win["res_target"] == 1).any()              # a frame that hosts nothing and is still observed
    assert (cnt[::3] == 0).all() and 3 * (cnt == 0).sum() >= win["np"]
    assert 4 <= outlier.sum() <= 8
    for p in ("host0", "rand10", "all"):
        f = MP.flags(win, p).astype(bool)
        kinds = [(f & (cnt == 0)).sum(), (f & outlier).sum(), (f & (cnt > 0) & ~outlier).sum()]
        print(p, "flagged: without residuals, with an OUTLIER residual, plain", kinds)
        assert min(kinds) >= 1
        if p != "all":
            g = ~f
            assert min((g & (cnt == 0)).sum(), (g & outlier).sum(), (g & (cnt > 0) & ~outlier).sum()) >= 1


def test_following_iteration_and_orthogonalised_references(oracle):
    """what the device's other bars come from: the float oracle's distance on the iteration after the marginalisation, and on HM / bM with
    SOLVER_ORTHOGONALIZE_POINTMARG / _FULL set"""
    for c in MP.FOLLOW_CASES:
        for p in MP.FOLLOW_PATTERNS:
            print("%-16s %-7s" % (c, p), {k: "%.2e" % v for k, v in MP.reference(oracle, c, p)[0]["follow"].items()})
    fb = MP.follow_bars(oracle)
    print("max / median:", {k: ("%.2e" % v[0], "%.2e" % v[1]) for k, v in fb.items()})
    assert all(0 < fb[k][1] <= fb[k][0] for k in fb)
    for c in MP.ORTH_CASES:
        plain = MP.reference(oracle, c, "host0")[1]
        for b in MP.ORTH_BITS:
            f32, f64 = MP.reference(oracle, c, "host0", b)
            acts = not np.array_equal(f64["HM"], plain["HM"])
            print("%-16s bits %2d e_H %.2e e_b %.2e differs from the plain prior: %s" % (c, b, f32["e_H"], f32["e_b"], acts))
            # POINTMARG alone with frame 0 in the window is the plain statement (EnergyFunctional.cpp:711-723)
            assert acts == (not (b == MP.ORTH_POINTMARG and c == "nf4"))
    E_H, E_b = MP.orth_bars(oracle)
    print("orthogonalised: E_H %.3e E_b %.3e" % (E_H, E_b))
    assert 0 < E_H <= 1e-5 and E_b <= 2e-6


def test_additivity_defect_of_the_float_oracle(oracle):
    for c in MP.ADD_CASES:
        win = MP.window(c)
        a, b, u = MP.additivity_flags(win)
        defect, H64 = MP.additivity_reference(oracle, c)
        print(c, "A", int(a.sum()), "B", int(b.sum()), "float oracle's whitened defect %.2e" % defect)
        assert a.any() and b.any() and not (a & b).any() and np.array_equal(u, a | b)
        assert 0 < defect <= 2e-5                       # three calls, each within E_H of its truth, and the truth is additive to rounding
