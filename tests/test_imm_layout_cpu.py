"""The ctx-free rules of the device-resident immature points (csrc/imm_layout.h: the member table of a point, the remove order of
activatePointsMT STEP 5 and its closed form as sdso_imm_activate's kernels compute it) checked on the CPU: csrc/test_imm_layout.cpp is a
stand-alone program with its own assertions; this test compiles it with the host compiler and runs it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")


def test_imm_layout_program(tmp_path):
    exe = str(tmp_path / "test_imm_layout")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", os.path.join(CSRC, "test_imm_layout.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "imm_layout ok" in r.stdout
