"""The bookkeeping of shared device blocks (csrc/share.h: holder count, exported mark, completion events, write in place or detach)
checked on the CPU: csrc/test_share.cpp is a stand-alone program that runs the header on a backend which only logs — four threads export,
import, detach and release blocks in random order, and the log must show every buffer freed exactly once, no free and no granted write
ahead of a completion event of that block, and every unexported block written in place.  This test compiles it with the host compiler
and runs it plain, under the address / undefined-behaviour sanitizers and under the thread sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ not found")

TSAN = ["-g", "-fsanitize=thread"]
PROBE = "#include <thread>\nstatic int x;\nint main() { std::thread t([] { x = 1; }); t.join(); return x - 1; }\n"


def _build(src, exe, flags):
    return subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-pthread"] + flags + [src, "-o", exe],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)


def _run(exe):
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], TSAN],
                         ids=["plain", "sanitizers", "tsan"])
def test_share_program(tmp_path, flags):
    if flags is TSAN:
        # the thread sanitizer needs a kernel / address-space layout it supports: a three-line threaded program built the same way decides
        probe = tmp_path / "probe.cpp"
        probe.write_text(PROBE)
        r = _build(str(probe), str(tmp_path / "probe"), flags)
        if r.returncode != 0 or _run(str(tmp_path / "probe")).returncode != 0:
            pytest.skip("a trivial threaded program does not run under -fsanitize=thread on this machine")
    exe = str(tmp_path / "test_share")
    r = _build(os.path.join(CSRC, "test_share.cpp"), exe, flags)
    assert r.returncode == 0, r.stdout[-4000:]
    r = _run(exe)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "share ok" in r.stdout
