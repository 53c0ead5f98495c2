"""The device buffer pool's ordering rule (csrc/pool.h, and share.h's drop_pooled) checked on the CPU: csrc/test_pool.cpp is a stand-alone
program that runs the headers on a backend which only logs — four threads build, export, import, detach, drop, acquire, trim and release
against one pool, under a cap that is never reached and under one that is often exceeded; before that the overflow path is walked step
by step on one thread (a cap filled with buffers whose events are pending, then one more), so that it does not hang on the schedule.  The log must show no buffer handed out
twice without a park in between, every hand-out behind a stream wait for each event of the buffer, no free ahead of the completion of
those events, no host wait under the cap, parked_bytes within the cap, every buffer freed and every event destroyed once, and the old
drop path for blocks without a pool.  This test compiles it with the host compiler and runs it plain, under the address /
undefined-behaviour sanitizers and under the thread sanitizer.  (csrc/test_share.cpp, which knows nothing of pools, must still build
against the extended share.h: tests/test_share_cpu.py.)"""
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
def test_pool_program(tmp_path, flags):
    if flags is TSAN:
        # the thread sanitizer needs a kernel / address-space layout it supports: a three-line threaded program built the same way decides
        probe = tmp_path / "probe.cpp"
        probe.write_text(PROBE)
        r = _build(str(probe), str(tmp_path / "probe"), flags)
        if r.returncode != 0 or _run(str(tmp_path / "probe")).returncode != 0:
            pytest.skip("a trivial threaded program does not run under -fsanitize=thread on this machine")
    exe = str(tmp_path / "test_pool")
    r = _build(os.path.join(CSRC, "test_pool.cpp"), exe, flags)
    assert r.returncode == 0, r.stdout[-4000:]
    r = _run(exe)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert all("pool ok (%s)" % k in r.stdout for k in ("overflow by hand", "under the cap", "cap exceeded"))


def test_size_classes(tmp_path):
    """pool.h's rounding: four classes per power of two, never below the request, at most a quarter above it (4 KiB granule below 32 KiB)"""
    src = tmp_path / "classes.cpp"
    src.write_text('#include "pool.h"\n#include <cstdio>\nint main() { for (size_t n = 1; n < (size_t)1 << 24; n += 1 + n / 7) {'
                   ' const size_t r = sdso::pool::round_up(n); if (r < n || (n >= 32768 && r > n + n / 4) || (n < 32768 && r >= n + 4096) ||'
                   ' sdso::pool::round_up(r) != r) { std::printf("bad %zu -> %zu\\n", n, r); return 1; } } std::puts("classes ok"); return 0; }\n')
    exe = str(tmp_path / "classes")
    r = _build(str(src), exe, ["-I", CSRC])
    assert r.returncode == 0, r.stdout[-4000:]
    r = _run(exe)
    assert r.returncode == 0 and "classes ok" in r.stdout, r.stdout[-2000:]
