"""tests/flag_points_ref.py on the CPU oracle's post-state (orc_ba_optimize, 6 iterations, orc_ba_get_post_state) of the three windows the
GPU test of sdso_ba_flag_points runs on: the decisions it produces there are the recorded ones, and they cover what the GPU comparison
needs — every code but DROP_NEGATIVE at least five times per case, every clause of PointHessian::isOOB deciding at least five times,
a point that leaves only because its host is flagged, a point that keeps seven residuals."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import flag_points_ref as ref


@pytest.fixture(scope="module")
def oracle_results(oracle):
    out = {}
    for name in ref.CASES:
        win, frame_marg, last_gone = ref.make_case(name)
        W, keep = abi.make_ba_window(win, dI_list=[p[0] for p in win["pyrs"]])
        h = oracle.orc_ba_create(C.byref(W))
        res = abi.BAOptResult()
        oracle.orc_ba_optimize(h, 6, None, None, None, C.byref(res))
        P, post = abi.make_post_state(win["nf"], win["np"], win["nr"])
        oracle.orc_ba_get_post_state(h, C.byref(P))
        oracle.orc_ba_destroy(h)
        out[name] = (win, post, frame_marg, last_gone, ref.flag_points(win, post, frame_marg, last_gone, minIdepthH_marg=ref.median_hessian(post)))
    return out


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_reference_on_oracle_post_state(oracle_results, name):
    win, post, frame_marg, last_gone, r = oracle_results[name]
    print(name, "np", win["np"], "codes", r["counts"].tolist(), "isOOB clauses", np.bincount(r["clause"], minlength=4)[1:].tolist(),
          "host-only", int(r["host_only"].sum()), "n >= 7", int((r["n"] >= 7).sum()), "n == 0", int((r["n"] == 0).sum()))
    assert win["np"] == ref.CASES[name]["nf"] * ref.CASES[name]["pts_per_kf"]
    assert r["counts"].sum() == win["np"] and np.array_equal(r["host_counts"].sum(0), r["counts"])
    assert np.array_equal(r["host_counts"].sum(1), np.bincount(win["host"], minlength=win["nf"]))
    ref.check_coverage(name, r)
    assert tuple(r["counts"].tolist()) == ref.CASES[name]["oracle_codes"]


def test_reference_coverage_over_the_cases(oracle_results):
    assert sum(int(v[4]["counts"][ref.DROP_NEGATIVE]) for v in oracle_results.values()) >= 1
    win, post, frame_marg, last_gone, r = oracle_results["A"]
    neg = np.nonzero(r["decision"] == ref.DROP_NEGATIVE)[0]
    assert len(neg) == 1 and post["idepth"][neg[0]] < -0.01                      # far from zero: not a rounding matter
    assert np.bincount(r["clause"], minlength=4)[1:].tolist() == [11, 99, 10]
    assert int(r["host_only"].sum()) == 43 and int((r["n"] >= 7).sum()) == 22 and int((r["n"] == 0).sum()) == 51
    # the caller's history matters: without it the decisions differ
    r0 = ref.flag_points(win, post, frame_marg, None, minIdepthH_marg=ref.median_hessian(post))
    assert (r0["decision"] != r["decision"]).sum() >= 5
    # and so do the residuals on toRemove: counting them as alive changes n
    post2 = dict(post); post2["toRemove"] = np.zeros_like(post["toRemove"])
    r2 = ref.flag_points(win, post2, frame_marg, last_gone, minIdepthH_marg=ref.median_hessian(post))
    assert (r2["decision"] != r["decision"]).sum() >= 5
