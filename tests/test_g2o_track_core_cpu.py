"""csrc/g2o_track_core.h — one try of the fork-live trackNewestCoarse as a state machine over its evaluations, the text k_g2o_track_lm
walks on the device — on the CPU: csrc/test_g2o_track_core.cpp, a stand-alone program that drives the core with closed-form evaluators
and holds it to g2o_lm::run (csrc/g2o_lm.h) on the same callbacks, compiled with the host compiler and run, plain and under the address
/ undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="g++ not found")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_g2o_track_core_program(tmp_path, flags):
    exe = str(tmp_path / "test_g2o_track_core")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_g2o_track_core.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "g2o_track_core ok" in r.stdout
