"""The contract of the buffers a ctx owns alone (csrc/devbuf.h) checked on the CPU: csrc/test_devbuf.cpp is a stand-alone program that
runs the header on a backend which only logs, and whose k-th allocation can be told to fail.  From the log and from the objects' state
it asserts: no backend call within capacity; a first reserve without a stream wait; a growth as wait on the given stream, free, alloc of
exactly `grown` elements; an empty buffer after a failed growth and a fresh allocation on the next, smaller, request; the group rule for
three buffers under one count with the failure at the second and at the third member; moves that empty their source and free the
destination's block once; frees on erasing a std::map entry; reset behind a wait; the pinned space on the pinned calls alone; and, after
every scenario, exactly one free per allocation.  This test compiles it with the host compiler and runs it plain and under the address /
undefined-behaviour sanitizers.  Nothing runs on the GPU and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_devbuf_program(tmp_path, flags):
    exe = str(tmp_path / "test_devbuf")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_devbuf.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "warning" not in r.stdout, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "devbuf ok" in r.stdout
