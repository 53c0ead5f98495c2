"""csrc/g2o_lba_core.h — what the fork-live window optimiser decides between its evaluations, the text k_lbar_ctl (g2o_lba_resident.hip)
walks on the device — on the CPU: csrc/test_g2o_lba_core.cpp, a stand-alone program that drives the controller with closed-form
evaluators and holds it to g2o_lm::run (csrc/g2o_lm.h) on the same callbacks bit for bit (all five stop reasons), and holds the core's
reduced-system assembly and solve to LbaProblem::trial's assembly with solveLdlt on random block-arrow systems (1..8 frames, hosts
without a slot, lambda 1e-9 .. 1e8, condition numbers 1 .. 6e8), bit for bit: the solver is solveLdlt's algorithm.  Compiled with the
host compiler and run, plain and under the address / undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="g++ not found")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_g2o_lba_core_program(tmp_path, flags):
    exe = str(tmp_path / "test_g2o_lba_core")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_g2o_lba_core.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "g2o_lba_core ok" in r.stdout and "bit for bit" in r.stdout
