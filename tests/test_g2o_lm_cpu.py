"""csrc/g2o_lm.h — g2o's Levenberg-Marquardt control, the loop of sdso_g2o_lba_optimize — on the CPU: csrc/test_g2o_lm.cpp, a
stand-alone program over a small dense least-squares problem and scripted chi2 sequences, compiled with the host compiler and run,
plain and under the address / undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="g++ not found")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_g2o_lm_program(tmp_path, flags):
    exe = str(tmp_path / "test_g2o_lm")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_g2o_lm.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "g2o_lm ok" in r.stdout
