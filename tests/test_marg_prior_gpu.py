"""sdso_ba_marginalize_points against the f64-ACCUMULATOR truth (orc_set_acc64), two to eight keyframes.

HM / bM are what outlives a window: they pass through marginalizeFrame into the next window's prior and compound over the sequence.  The
call runs kernels the other truth tests do not reach — k_ba_accum_top in mode 2 with the point filter, k_ba_fold_top, k_ba_sc_host<false, *>
with shift = 0 / mm = 1, k_ba_stitch_pre, k_ba_stitch<0>, then k_ba_prior_add or k_ba_prior_orth — and tests/test_ba_marg_gpu.py holds it to the
float oracle at 1e-4 at one shape.  Here every bar is derived from the float oracle's OWN distance to the truth (tests/marg_prior_cases.py,
asserted on the CPU by tests/test_marg_prior_ref.py), never from the device:

  * HM / bM (whitened by the truth's diagonal, e_H / e_b of marg_prior_cases): device <= 2 * E_H = 7.9e-6 and 2 * E_b = 2.2e-6, where E_H
    / E_b are the float oracle's largest distances over the ten windows and five flag patterns (the old bar: 1e-4 on both); and over all
    (window, pattern) pairs the device's median is not above the float oracle's;
  * structure, exact: the same zeros as the truth, an unflagged call leaves the prior bit-identical, residual state / isActive / JpJdF
    bit-equal to the float oracle's, resInM the oracle's count;
  * localisation: the packed accumulator block right after the call against orc_ba_get_accumulators_f64 (the oracle's marginalisation
    accumulates into the set its getters read), section by section at the 3e-7 of tests/test_ba_f64_truth_gpu.py, empty bins empty;
  * additivity, independent of the oracle's arithmetic: HM(A u B) - HM(A) - HM(B) for disjoint flag sets is zero in exact arithmetic; the
    device's whitened defect is at most twice the float oracle's;
  * the iteration after the marginalisation (the linearised pass accumulateLF, TAIL_TOPL): stitched H, b, x and the point steps against
    the truth, per window <= 2 * the float oracle's largest distance, median <= the float oracle's median; point terms bit-equal;
  * SOLVER_ORTHOGONALIZE_POINTMARG / _FULL (k_ba_prior_orth) with and without frame 0, at twice the float oracle's distance in that mode.

Measured on MI355X (tests/diag/marg_prior_errors.py -> profiles/marg_prior_errors.txt): see the figures quoted in each test."""
import numpy as np
import pytest

import marg_prior_cases as MP

pytestmark = pytest.mark.gpu

_dev = {}


def _device(ctx, oracle, case, pattern, bits=0):
    """the device's run of one (window, pattern, solver bits), once per process"""
    key = (case, pattern, bits)
    if key not in _dev:
        win = MP.with_solver_bits(MP.window(case), bits) if bits else MP.window(case)
        follow = bits == 0 and case in MP.FOLLOW_CASES and pattern in MP.FOLLOW_PATTERNS
        r = MP.device_marginalize(ctx, win, MP.flags(win, pattern), follow=follow)
        f64 = MP.reference(oracle, case, pattern, bits)[1]
        r["e_H"], r["e_b"] = MP.e_H(r["HM"], f64["HM"]), MP.e_b(r["bM"], f64["HM"], f64["bM"])
        if follow:
            r["follow"] = MP.follow_distances(r, f64)
        _dev[key] = r
    return _dev[key]


@pytest.fixture(scope="module")
def bars(oracle):
    E_H, E_b = MP.bars(oracle)
    assert 0 < E_H <= 1e-5 and 0 < E_b <= 2e-6          # (tests/test_marg_prior_ref.py: the derived bars can never silently widen)
    return E_H, E_b


@pytest.mark.parametrize("case", MP.CASES)
def test_prior_against_f64_truth(gpu_ctx, oracle, bars, case):
    """Measured on MI355X: device e_H 5.3e-8..2.2e-6, e_b 1.7e-8..3.3e-7 over the forty (window, pattern) pairs that flag a point; float oracle
    8.6e-8..4.0e-6 and 3.9e-8..1.1e-6.  Accumulator sections of the marginalisation pass: device 4.7e-9..1.3e-7, float oracle 7.1e-9..7.6e-7."""
    E_H, E_b = bars
    win = MP.window(case)
    HM0, bM0 = MP.prior_in(win)
    for pattern in MP.PATTERNS:
        f32, f64 = MP.reference(oracle, case, pattern)
        g = _device(gpu_ctx, oracle, case, pattern)
        secs, (cnt_g, cnt_t) = MP.section_errors(g["acc"], f64["acc"], win["nf"])
        print("%-16s %-7s e_H device %.2e oracle_f32 %.2e (bar %.2e) | e_b device %.2e oracle_f32 %.2e (bar %.2e) | sections %s"
              % (case, pattern, g["e_H"], f32["e_H"], 2 * E_H, g["e_b"], f32["e_b"], 2 * E_b, " ".join("%s %.1e" % (n, e) for n, e, _ in secs)))
        assert g["e_H"] <= 2 * E_H, (pattern, g["e_H"], f32["e_H"])
        assert g["e_b"] <= 2 * E_b, (pattern, g["e_b"], f32["e_b"])
        assert np.array_equal(g["HM"] == 0, f64["HM"] == 0), pattern                  # the same frames touched
        if pattern == "none":
            assert np.array_equal(g["HM"], HM0) and np.array_equal(g["bM"], bM0)      # nothing flagged: HM += 0.25 * (0 - 0)
            assert bM0.any() or not g["bM"].any()
        assert np.array_equal(g["state"], f32["state"]) and np.array_equal(g["act"], f32["act"]) and np.array_equal(g["jp"], f32["jp"]), pattern
        assert g["resInM"] == f64["resInM"] == f32["resInM"], (pattern, g["resInM"], f64["resInM"])
        # localisation: the marginalisation pass' sums, before the stitch
        for name, err, empty_ok in secs:
            assert err <= 3e-7, (pattern, name, err)
            assert empty_ok, (pattern, name)                                          # bins empty in the truth are empty on the device
        assert np.array_equal(cnt_g, cnt_t), (pattern, cnt_g, cnt_t)


def test_prior_distribution_is_not_above_the_float_oracle(gpu_ctx, oracle):
    """Over all (window, pattern) pairs: the device's median distance from the truth is not above the float oracle's — the distribution form
    of test_ba_f64_truth_gpu.py::test_device_noise_is_the_cpu_float_noise.  Measured on MI355X: e_H median device 1.3e-7 against 4.1e-7,
    e_b 7.0e-8 against 1.2e-7."""
    dev, orc = [], []
    for case in MP.CASES:
        for pattern in MP.PATTERNS:
            dev.append(_device(gpu_ctx, oracle, case, pattern))
            orc.append(MP.reference(oracle, case, pattern)[0])
    for k in ("e_H", "e_b"):
        md, mo = np.median([r[k] for r in dev]), np.median([r[k] for r in orc])
        print("%s median: device %.2e, float oracle %.2e; max: device %.2e, float oracle %.2e" % (k, md, mo, max(r[k] for r in dev), max(r[k] for r in orc)))
        assert md <= mo, (k, md, mo)


@pytest.mark.parametrize("case", MP.ADD_CASES)
def test_prior_is_additive_over_disjoint_flag_sets(gpu_ctx, oracle, case):
    """Every flagged point adds its own terms to M and Msc, so HM(A u B) - HM(A) - HM(B) = 0 in exact arithmetic (zero incoming prior; A the
    oldest frame's points, B the random 10 % outside it), whatever the oracle computes.  A point filter that drops or doubles a chunk fails
    here.  Measured on MI355X: whitened defect device 6.3e-8 / 7.5e-8 against the float oracle's 3.0e-7 (nf4) / 6.6e-8 (nf2_two_chunks)."""
    win = MP.window(case)
    a, b, u = MP.additivity_flags(win)
    defect_o, H64 = MP.additivity_reference(oracle, case)
    HA, HB, HU = [MP.device_marginalize(gpu_ctx, win, f, want_acc=False)["HM"] for f in (a, b, u)]
    defect_g = MP.whitened_defect(HU, HA, HB, H64)
    print("%s: additivity defect device %.2e, float oracle %.2e" % (case, defect_g, defect_o))
    assert np.abs(HA).max() > 0 and np.abs(HB).max() > 0
    assert defect_g <= 2 * defect_o, (defect_g, defect_o)


@pytest.mark.parametrize("case", MP.FOLLOW_CASES)
def test_iteration_after_the_marginalisation_against_f64_truth(gpu_ctx, oracle, case):
    """linearize, applyRes, accumulate (accumulateAF + accumulateLF on the residuals fixLinearizationF froze) and solve after the
    marginalisation, against the same on the truth.  Per window the device is within twice the float oracle's LARGEST distance over these
    windows (H 2.5e-6, b 8.9e-9, x 2.3e-5, point steps 1.6e-4).  The fixed bars of test_ba_f64_truth_gpu.py (H 1e-7, x 1e-5) are printed, not
    asserted: the float oracle itself misses them at two and three keyframes.  Measured on MI355X: device H 1.9e-8..5.2e-7, b 7.5e-11..2.0e-9, x 6.5e-7..3.3e-6,
    point steps 4.9e-6..2.9e-5; the device meets x 1e-5 on all ten pairs and H 1e-7 on all but the two of nf2_two_chunks (1.3e-7, 5.2e-7)."""
    fb = MP.follow_bars(oracle)
    for pattern in MP.FOLLOW_PATTERNS:
        f32, f64 = MP.reference(oracle, case, pattern)
        g = _device(gpu_ctx, oracle, case, pattern)
        print("%-16s %-7s" % (case, pattern), " | ".join("%s device %.2e oracle_f32 %.2e (bar %.2e)" % (k, g["follow"][k], f32["follow"][k], 2 * fb[k][0]) for k in fb),
              "| fixed bars H 1e-7: %s, x 1e-5: %s" % (g["follow"]["H"] <= 1e-7, g["follow"]["x"] <= 1e-5))
        for k in fb:
            assert g["follow"][k] <= 2 * fb[k][0], (pattern, k, g["follow"][k], fb[k][0])
        for a, b in zip(f32["terms"], g["terms"]):
            assert np.array_equal(a, b), pattern                                     # HdiF, bdSumF, Hdd / bd / Hcd incl. the accLF parts: bit-exact
        assert np.abs(g["x"]).max() > 0 and np.isfinite(g["x"]).all()


def test_iteration_after_the_marginalisation_distribution(gpu_ctx, oracle):
    """over the ten (window, pattern) pairs of the following iteration the device's median distance is not above the float oracle's.
    Measured on MI355X, device against float oracle: H 4.6e-8 / 1.6e-7, b 2.9e-10 / 9.2e-10, x 1.8e-6 / 5.9e-6, point steps 9.6e-6 / 3.3e-5."""
    fb = MP.follow_bars(oracle)
    rows = [_device(gpu_ctx, oracle, c, p)["follow"] for c in MP.FOLLOW_CASES for p in MP.FOLLOW_PATTERNS]
    for k in fb:
        md = float(np.median([r[k] for r in rows]))
        print("%s median: device %.2e, float oracle %.2e" % (k, md, fb[k][1]))
        assert md <= fb[k][1], (k, md, fb[k][1])


@pytest.mark.parametrize("bits", MP.ORTH_BITS)
@pytest.mark.parametrize("case", MP.ORTH_CASES)
def test_orthogonalised_prior_against_f64_truth(gpu_ctx, oracle, case, bits):
    """EnergyFunctional.cpp:707-731 through k_ba_prior_orth: the points' H / b projected off the gauge when frame 0 has left the window
    (SOLVER_ORTHOGONALIZE_POINTMARG), the whole prior projected (SOLVER_ORTHOGONALIZE_FULL), both.  The bar is twice the float oracle's
    largest distance WITH THAT MODE SET (E_H 4.6e-7, E_b 3.8e-7: tighter than the plain windows' bar).  Measured on MI355X: device e_H 1.9e-7..3.5e-7,
    e_b 5.6e-8..8.3e-8; float oracle 3.4e-7..4.6e-7, 2.1e-7..3.8e-7."""
    E_H, E_b = MP.orth_bars(oracle)
    assert E_H <= MP.bars(oracle)[0]
    f32, f64 = MP.reference(oracle, case, "host0", bits)
    g = _device(gpu_ctx, oracle, case, "host0", bits)
    print("%-16s bits %2d e_H device %.2e oracle_f32 %.2e (bar %.2e) | e_b device %.2e oracle_f32 %.2e (bar %.2e)"
          % (case, bits, g["e_H"], f32["e_H"], 2 * E_H, g["e_b"], f32["e_b"], 2 * E_b))
    assert g["e_H"] <= 2 * E_H and g["e_b"] <= 2 * E_b, (g["e_H"], g["e_b"])
    assert np.array_equal(g["HM"] == 0, f64["HM"] == 0)
    assert np.array_equal(g["state"], f32["state"]) and np.array_equal(g["act"], f32["act"]) and np.array_equal(g["jp"], f32["jp"])
    assert g["resInM"] == f64["resInM"]
