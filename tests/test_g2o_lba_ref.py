"""tests/g2o_lba_ref.py — the NumPy statement of the fork-live window optimiser that sdso_g2o_lba_optimize is held to — on the CPU.

The reference must take every branch it can, and it must take them with a margin, so that the integer outcomes of a second
implementation that differs in the order of its f64 sums are comparable: every trial's |rho| >= 1e-4, every gain at least 1e-4 away from
the threshold.  A case that violates a margin is replaced, not exempted.  What the runs came to when the cases were chosen:

  A  1168 residuals, 1 at level 1; trials 5 / 3 / 6; ends on the iteration cap
  B  three iterations, stops on gain (1.9e-4)
  C  four iterations, one of 7 trials with lambda to 8e6, stops on gain (4.2e-4)
  D  full window of 8 hosts, iteration cap
  E  C with lambda0 1e-9: 9 trials in iteration 0
  F  A with the doctored points of test_gpu_lba_edge_bit_exact: 25 inactive edges, 5 more reach level 1 during the call; gain 8.6e-4
  G  B with host 1's points out of the image: 79 inactive edges, a host without an active edge
"""
import numpy as np
import pytest

import g2o_lba_ref as ref

GAIN_TH = 1e-3


@pytest.fixture(scope="module")
def runs(oracle):
    return {n: ref.reference(oracle, n) for n in ref.CASES}


def test_margins(runs):
    for n, r in runs.items():
        assert r["rhos"] and min(abs(x) for x in r["rhos"]) >= 1e-4, (n, min(abs(x) for x in r["rhos"]))
        assert all(abs(g - GAIN_TH) >= 1e-4 for g in r["gains"]), (n, r["gains"])
        assert all(np.isfinite(r["lambdas"])) and all(np.isfinite(r["chi2"]))


def test_every_branch_is_taken(runs):
    A, B, C_, D, E, F, G = [runs[n] for n in "ABCDEFG"]
    assert ref.case("A")["nr"] == 1168 and int((~A["active"]).sum()) == 1
    assert A["trials"] == [5, 3, 6] and A["stop"] == ref.STOP_ITERATIONS and A["iterations"] == 3
    assert B["iterations"] == 3 and B["stop"] == ref.STOP_GAIN and B["iterations"] < ref.case("B")["iterations"]
    assert C_["iterations"] == 4 and 7 in C_["trials"] and max(C_["lambdas"]) > 1e6 and C_["stop"] == ref.STOP_GAIN
    assert len(D["hosts"]) == 8 and D["stop"] == ref.STOP_ITERATIONS
    assert E["trials"][0] == 9
    for r in runs.values():
        assert r["accepted"] > 0 and r["rejected"] > 0                         # rejected and accepted trials
        assert r["accepted"] + r["rejected"] == sum(r["trials"]) == len(r["rhos"])
        assert r["n_active"] == int(r["active"].sum()) > 0
    # inactive edges, edges that reach level 1 only during the call, a host without an active edge
    assert int((~F["active"]).sum()) >= 20 and int(F["level"].sum()) > int((~F["active"]).sum())
    assert set(np.unique(F["state"])) == {0, 1, 2}
    assert G["hosts"] == [0, 2] and not np.any(G["active"][ref.case("G")["host"] == 1])


def test_the_loop_lowers_the_robust_chi2(oracle, runs):
    for n, r in runs.items():
        c = ref.case(n)
        first = ref.optimize(oracle, c, max_iterations=0)
        assert first["iterations"] == 0 and np.array_equal(first["idepth"], c["idepth"])
        assert r["chi2_final"] < first["chi2_final"]
        assert all(b <= a for a, b in zip([first["chi2_final"]] + r["chi2"][:-1], r["chi2"]))
        # untouched: inactive edges' idepths, hosts without an active edge
        assert np.array_equal(r["idepth"][~r["active"]], c["idepth"][~r["active"]])
        for h in range(c["nf"]):
            if h not in r["hosts"]:
                assert np.array_equal(r["Twh"][h][0], c["Twh"][h][0]) and r["host_aff"][h] == c["host_aff"][h]


def test_schur_solution_equals_the_full_system(oracle):
    """one trial of case C with the Schur complement against the dense solve over all 8 nh + 4 + nr unknowns"""
    c = ref.case("C")
    o = ref.oracle_eval(oracle, c, c["Twh"], c["host_aff"], c["cam"], c["idepth"])
    act = o["lvl"] == 0
    nr, nh = c["nr"], c["nf"]
    n = 8 * nh + 4
    lam = 6.4        # 0.1 * 2 * 4 * 8: where the run of C accepts its first step
    e = o["error"]; J = o["J"].copy(); J[~act] = 0
    e2 = (e ** 2).sum(1)
    rho1 = np.where(act, np.where(e2 <= 81.0, 1.0, 9.0 / np.sqrt(np.maximum(e2, 1e-300))), 0.0)
    H = np.zeros((n + nr, n + nr)); b = np.zeros(n + nr)
    for r in range(nr):
        ix = np.array([8 * c["host"][r] + k for k in range(8)] + [n + r] + [8 * nh + k for k in range(4)])
        H[np.ix_(ix, ix)] += rho1[r] * J[r].T @ J[r]
        b[ix] -= rho1[r] * J[r].T @ e[r]
    x_full = np.linalg.solve(H + lam * np.eye(n + nr), b)
    # the reference's first trial, read off its first rho: rebuild it through optimize() with one iteration and one trial
    r1 = ref.optimize(oracle, c, max_iterations=1, lambda_init=lam, max_trials=1)
    assert r1["accepted"] == 1
    assert np.allclose(r1["cam"] - c["cam"], x_full[8 * nh:n], rtol=1e-6, atol=1e-12)
    assert np.allclose((r1["idepth"] - c["idepth"])[act], x_full[n:][act], rtol=1e-6, atol=1e-12)
    assert np.allclose(r1["host_aff"][1][1] - c["host_aff"][1][1], x_full[8 + 7], rtol=1e-6, atol=1e-12)
