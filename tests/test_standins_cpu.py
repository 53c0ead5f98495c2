"""The stand-in types and the graph builder of the shim's test drivers (host/standins.h, host/driver_io.h) where they own memory, checked
on the CPU: host/test_standins.cpp is a stand-alone program that writes a small window, builds the pointer graph, runs dropResidual /
removePoint / dropPointsF and asserts the index invariants after every step; this test compiles it with the host compiler and runs it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo-dso-g2o_amd", "host")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")


def _compile_and_run(tmp_path, name, says):
    exe = str(tmp_path / name)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", os.path.join(HOST, name + ".cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert says in r.stdout


def test_standins_program(tmp_path):
    _compile_and_run(tmp_path, "test_standins", "standins ok")


def test_shim_marshal_program(tmp_path):
    """The shim's shared marshalling rules (host/shim/marshal.h) in host/test_shim_marshal.cpp: the immature-point columns with their
    gather, the ABI struct and the three scatters; the (a b + c d) + e f order of the 3 x 3 float products, bit for bit; the per-level
    intrinsics at 1232 x 368 over 6 levels in double and in float.  It links without the device library: the header calls nothing of it."""
    _compile_and_run(tmp_path, "test_shim_marshal", "marshal ok")
