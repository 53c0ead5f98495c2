"""Static check of where k_ba_lin_fused waits for memory: ba.hip is compiled for gfx950 with the Makefile's flags to a listing
(no GPU needed) and tools/isa_waits.py walks it.

The kernel's life is waiting (a workgroup lives ~41 us and issues ~7 us of VALU work), so what it is priced by is the number of
`s_waitcnt vmcnt` that stand between a memory round trip and the next one.  Asserted for k_ba_lin_fused<true> and <false>:

  * no flat_ instruction: every access goes through gld / gst / uld (ba_kernels.h) or the taps' raw buffer, so waits on memory are
    counted ones and a wait in front of an LDS read does not cover the load issued before it;
  * the 32 tap loads come as four batches of eight with no vmcnt wait inside a batch;
  * waits with loads outstanding: at most 3 before the first tap load (the design needs two: the residual's scalars, the point),
    exactly 4 in the gather (one per batch), at most 1 from the first Jacobian store to the first barrier (none is needed);
  * registers: <true> within 168 VGPRs, <false> within 128; no scratch; 40 KB of LDS.  Both variants are launched for four workgroups
    per CU (`__launch_bounds__(BA_BLOCK, 4)`), so what the code itself relies on is tighter and asserted as well: at most 128 VGPRs and
    an occupancy of 4 waves per SIMD in the compiler's report, for both.

Measured on the parent of this change with the same tool (k_ba_lin_fused<true>; <false> the same but for the registers):
104 flat_ instructions; tap batches [1, 1, 1, 1, 1, 1, 1, 1, 8, 8, 8] (the first batch waited vmcnt(0) behind every load: its image
pointer came from a vector load that only those branches waited for); 11 waits with loads outstanding before the first tap, 11 in
the gather, 3 up to the first barrier and 3 more behind it (r_orig, r_jsel, the read-back of r_newEnergy); 149 VGPRs, <false> 128
VGPRs and 12 bytes of scratch.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

KERNELS = {"true": ("k_ba_lin_fusedILb1", 168), "false": ("k_ba_lin_fusedILb0", 128)}


def makefile_flags():
    """FLAGS of csrc/Makefile with its variables at their defaults"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*=\s*(.*)$", mk, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    return flags.replace("$(EXTRA)", "").replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "ba.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-S", "ba.hip", "-o", out]
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


@pytest.fixture(scope="module", params=sorted(KERNELS))
def report(request, listing):
    import isa_waits
    name, vgpr_budget = KERNELS[request.param]
    r = isa_waits.analyse(listing, name)
    r["vgpr_budget"] = vgpr_budget
    print("\nk_ba_lin_fused<%s>: VGPRs %s, scratch %s B, LDS %s B, flat %d, tap batches %s, waits front/gather/back %d/%d/%d" % (
        request.param, r["vgprs"], r["scratch_bytes"], r["lds_bytes"], len(r["flat"]), r["tap_batches"], r["waits_front"], r["waits_gather"], r["waits_back"]))
    for w in r["waits"]:
        print("  %-6s #%-5d %-32s loads outstanding %d" % (w["stretch"], w["index"], w["text"], w["loads_outstanding"]))
    return r


def test_no_flat_instruction(report):
    assert report["flat"] == []


def test_tap_batches(report):
    assert report["tap_loads"] == 32
    assert report["tap_batches"] == [8, 8, 8, 8]


def test_waits_with_loads_outstanding(report):
    assert report["waits_front"] <= 3
    assert report["waits_gather"] == 4
    assert report["waits_back"] <= 1


def test_register_budget(report):
    assert report["vgprs"] is not None and report["vgprs"] <= report["vgpr_budget"]
    assert report["vgprs"] <= 128 and report["occupancy"] == 4   # four workgroups of four waves per CU
    assert report["scratch_bytes"] == 0
    assert report["scratch"] == []
    assert report["lds_bytes"] == 40960
