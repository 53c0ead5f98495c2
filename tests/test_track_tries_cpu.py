"""The loop over the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511) as csrc/track_tries.h states it, on the CPU.

1. csrc/test_track_tries.cpp — a stand-alone program whose expectations are read off the reference — compiled with the host compiler
   and run, plain and under the address / undefined-behaviour sanitizers.
2. sdso_track_tries_replay (the ctx-free entry of the library) against tests/track_tries_ref.py, an independent Python statement of
   the loop over a mock tracker that replays event traces, on a few thousand seeded random lists: integers exactly, doubles bit for
   bit.  The lists must contain every situation the rules distinguish; the test counts them off the reference's outcomes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from sdso_amd import abi
import track_tries_cases as cases
import track_tries_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="g++ not found")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_track_tries_program(tmp_path, flags):
    exe = str(tmp_path / "test_track_tries")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_track_tries.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "track_tries ok" in r.stdout


def _situations(recs, tries, aff0, rmse, thr, want, seen_kinds):
    """which of the situations the rules distinguish this list contains, read off the reference's walk"""
    bound = [float("nan")] * 5                                   # achievedRes before try i: the reference on the prefix, never stopping
    for i, s in enumerate(want["seen"]):
        if s is None:
            break
        if i:
            bound = ref.track_new_coarse(recs[:i], tries[:i], aff0, [0.0] * 5, thr)["achievedRes"]
        ev = recs[i]["events"]
        if ev and all(np.isnan(b) for b in bound):
            seen_kinds.add("nan bounds")
        if s["abort_lvl"] >= 0:
            e = next(k for k, (lvl, res, _) in enumerate(ev) if res > 1.5 * bound[lvl])
            if e + 1 < len(ev) and ev[e + 1][0] == ev[e][0] and not ev[e + 1][1] > 1.5 * bound[ev[e][0]]:
                seen_kinds.add("first pass alone crosses")
            if e > 0 and ev[e - 1][0] == ev[e][0]:
                seen_kinds.add("second pass alone crosses")
            if want["haveOneGood"] and any(np.isfinite(s["lastResiduals"][l]) and bound[l] > s["lastResiduals"][l] for l in range(5)):
                seen_kinds.add("aborted try lowers a coarser bound")
        if s["good"] and not ref._isfinite_f(s["lastResiduals"][0]):
            seen_kinds.add("non-finite level-0 residual")
        if s["good"] and s["lastResiduals"][0] == bound[0]:
            assert s["winner"] == 0
            seen_kinds.add("residual equal to the bound")
    if want["haveOneGood"]:
        a0, t = want["achievedRes"][0], rmse[0] * thr
        if want["tryIterations"] < len(tries):
            seen_kinds.add("stopped")
        if a0 == t:
            seen_kinds.add("on the stop threshold")              # strict <: goes on
            assert want["tryIterations"] == len(tries)
        if 0.99 * t < a0 < t:
            seen_kinds.add("just below the stop threshold")      # stops
            assert want["seen"][want["tryIterations"] - 1] is not None and (want["tryIterations"] == len(tries) or want["seen"][want["tryIterations"]] is None)
    else:
        seen_kinds.add("no good try")


def test_replay_equals_the_python_loop():
    L = abi.load()
    rs = np.random.RandomState(436511)
    kinds = set()
    for it in range(4000):
        recs, tries, aff0, rmse, thr = cases.random_list(rs)
        want = ref.track_new_coarse(recs, tries, aff0, rmse, thr)
        R, T = cases.to_c(recs, tries)
        rc, out, rm = cases.replay(L, R, T, aff0, rmse, thr)
        assert rc == 0
        cases.assert_equal_to_ref(out, rm, R, want, what=it)
        if it < 1500:
            _situations(recs, tries, aff0, rmse, thr, want, kinds)
    need = {"nan bounds", "first pass alone crosses", "second pass alone crosses", "aborted try lowers a coarser bound", "non-finite level-0 residual",
            "residual equal to the bound", "stopped", "on the stop threshold", "just below the stop threshold", "no good try"}
    assert need <= kinds, need - kinds


def test_replay_refusals():
    """SDSO_ERR_ARG and nothing written: a null argument, ntries outside 1..64, a trace that cannot be one"""
    L = abi.load()
    rs = np.random.RandomState(5)
    recs, tries, aff0, rmse, thr = cases.random_list(rs)
    R, T = cases.to_c(recs, tries)
    a = abi.Aff(*aff0)
    ERR_ARG = -1

    def call(n=len(recs), T=T, a=C.byref(a), R=R, rm=True, out=True):
        o = abi.TrackTriesResult(); o.winner = 77
        m = (C.c_double * 5)(*rmse)
        before = bytes(R) if R is not None else b""
        rc = L.sdso_track_tries_replay(n, T, a, R, m if rm else None, thr, C.byref(o) if out else None)
        assert rc == ERR_ARG and o.winner == 77 and (bytes(R) if R is not None else b"") == before
        assert all(ref.same_double(x, y) for x, y in zip(m, rmse))

    call(T=None); call(a=None); call(R=None); call(rm=False); call(out=False)
    call(n=0); call(n=-3); call(n=65)
    for n_ev, lvl in ((7, 0), (-1, 0), (2, 5), (2, -1)):
        R2, _ = cases.to_c(recs, tries)
        R2[len(recs) - 1].trace.n = n_ev
        R2[len(recs) - 1].trace.lvl[1] = lvl
        call(R=R2)
    big = [dict(events=[(0, 5.0, (0.0, 0.0, 0.0))], end_good=1, end_pose=tries[0], end_aff=(0.0, 0.0))] * 64
    R3, T3 = cases.to_c(big, [tries[0]] * 64)
    assert cases.replay(L, R3, T3, aff0, [0.0] * 5, 1.5)[0] == 0
