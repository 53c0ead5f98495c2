"""The ctx-free host half of the BA window upload (csrc/ba_layout.h: validation, the stable pair sort, chunk / item work lists, the
per-point tables, and its composition with plan_window_edit) checked on the CPU: csrc/test_ba_layout.cpp is a stand-alone program with
its own window generator and assertions; this test compiles it with the host compiler and runs it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")


def test_ba_layout_program(tmp_path):
    exe = str(tmp_path / "test_ba_layout")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", os.path.join(CSRC, "test_ba_layout.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ba_layout ok" in r.stdout
