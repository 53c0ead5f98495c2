"""The per-point decision of FullSystem::removeOutliers / flagPointsForRemoval (csrc/ba_flag.h, what k_ba_flag_points evaluates per lane)
checked on the CPU: csrc/test_ba_flag.cpp is a stand-alone program whose expectations are read off the reference — every branch, each
clause of PointHessian::isOOB alone, the boundaries n = 2 / 3, numGoodResiduals = 3 / 4 / 14 / 15, idepth_hessian on the threshold,
idepth = -0.0f, nf = 2, a last_gone value beating a live residual.  This test compiles it with the host compiler and runs it, plain and
under the address / undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_ba_flag_program(tmp_path, flags):
    exe = str(tmp_path / "test_ba_flag")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_ba_flag.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ba_flag ok" in r.stdout
