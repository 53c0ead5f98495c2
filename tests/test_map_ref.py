"""tests/map_ref.py on the CPU oracle's post-state (orc_ba_optimize, 6 iterations, orc_ba_get_post_state) of the three windows of
tests/flag_points_ref.py — what the GPU tests of sdso_map_update / sdso_map_cloud rely on: with the quantile thresholds every keep
clause of refreshPC decides at least five points and at least fifty survive in each window, the recorded counts are met, the walking
loops leave list orders that differ from the window's, and every point ends in exactly one list."""
import ctypes as C

import numpy as np
import pytest

from sdso_amd import abi
import flag_points_ref as fref
import map_ref as ref


@pytest.fixture(scope="module")
def oracle_cases(oracle):
    out = {}
    for name in ref.CASES:
        win, frame_marg, last_gone = fref.make_case(name)
        W, keep = abi.make_ba_window(win, dI_list=[p[0] for p in win["pyrs"]])
        h = oracle.orc_ba_create(C.byref(W))
        res = abi.BAOptResult()
        oracle.orc_ba_optimize(h, 6, None, None, None, C.byref(res))
        P, post = abi.make_post_state(win["nf"], win["np"], win["nr"])
        oracle.orc_ba_get_post_state(h, C.byref(P))
        oracle.orc_ba_destroy(h)
        K4 = np.array(P.calib_value_scaled[:])
        out[name] = (win, post, K4, ref.case_on_post(name, win, post, frame_marg, last_gone))
    return out


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_thresholds_make_every_clause_decide(oracle_cases, name):
    win, post, K4, c = oracle_cases[name]
    th = ref.quantile_thresholds(c["frames"])
    r = ref.cloud(c["frames"], K4, mode=1, **th)
    dropped = tuple(int((r["clause"] == k).sum()) for k in (1, 3, 4, 5))
    kept = int((r["clause"] == 0).sum())
    status = tuple(sum(len(f["lists"][l]) for f in c["frames"]) for l in (1, 2, 3))
    print(name, "np", win["np"], "thresholds", th, "dropped (mode / scaled / abs / bs)", dropped, "kept", kept, "status", status)
    assert sum(status) == win["np"] == len(r["clause"])
    assert status == ref.CASES[name]["status"] == (int(c["decision"].tolist().count(0)), int(c["decision"].tolist().count(3)),
                                                   win["np"] - int(np.isin(c["decision"], (0, 3)).sum()))
    assert min(dropped) >= 5 and kept >= 50
    assert dropped == ref.CASES[name]["dropped"] and kept == ref.CASES[name]["kept"]
    assert r["first"][-1] == 8 * kept and r["kept"].sum() == kept and len(r["xyz"]) == len(r["rgb"]) == 8 * kept
    cand = np.concatenate([f["lists"][l] for f in c["frames"] for l in (1, 2)])
    assert (cand[:, 4] != 0).all()                                             # minBS decides on values, not on the zeros of a fresh point
    assert np.isfinite(r["xyz"]).all()


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_walks_permute_and_partition(oracle_cases, name):
    win, post, K4, c = oracle_cases[name]
    w = c["walk"]
    act = [p for l in w["active"] for p in l]
    assert sorted(act + w["gone"].tolist()) == list(range(win["np"]))
    host = np.asarray(win["host"])
    for h, l in enumerate(w["active"]):
        assert (host[l] == h).all()
    assert act != sorted(act)                                                  # the list order is not the window's
    assert (np.diff(w["gone"][host[w["gone"]] == 0]) < 0).any()                # nor is the push order
    # the swap-with-back of removeOutliers moves survivors: its result differs from a stable filter
    lists = ref.point_lists(win["host"], win["nf"])
    l1, g1 = ref.walk_remove_outliers(lists, c["decision"] == fref.DROP_NO_RESIDUAL)
    assert any(a != [p for p in b if c["decision"][p] != fref.DROP_NO_RESIDUAL] for a, b in zip(l1, lists))
    assert len(g1) == int((c["decision"] == fref.DROP_NO_RESIDUAL).sum()) >= 5


def test_modes_and_colours(oracle_cases):
    win, post, K4, c = oracle_cases["C"]
    th = ref.quantile_thresholds(c["frames"])
    n = {m: ref.cloud(c["frames"], K4, mode=m, **th) for m in (0, 1, 2, 3)}
    assert n[3]["first"][-1] == 0 and n[0]["first"][-1] > n[1]["first"][-1] > n[2]["first"][-1] > 0
    assert (n[2]["kept"][:, [0, 2, 3]] == 0).all() and (n[1]["kept"][:, [0, 3]] == 0).all() and (n[0]["kept"][:, 3] > 0).any()
    assert set(map(tuple, n[0]["rgb"].tolist())) == {(0, 255, 0), (0, 0, 255), (255, 0, 0)}
    assert (n[1]["rgb"][:, 0] == n[1]["rgb"][:, 1]).all() and len(np.unique(n[1]["rgb"])) > 20
    assert ref.grey([0, 255.9, np.nan, 256, -1, 1e10, 300.7]).tolist() == [0, 255, 0, 0, 255, 0, 44]
