"""The statements behind the keyframe's depth image, checked without a GPU.

* tests/depth_image_ref.py's level-0 map against synth.make_pc: inside [2,w-2) x [2,h-2) the positive pixels of the map, in raster order,
  are the level-0 template (u, v, idepth, colour), and every other pixel there is -1.  (The two-pixel border holds raw sums: no template
  ever shows them, only debugPlotIDepthMap's sort does.)
* csrc/test_depth_image.cpp, the CPU program over csrc/depth_image.h — the gather order against the literal scatter loop, makeJet3B at
  every case boundary and at NaN / +-inf, the radix key order against std::sort — plain and under the address / undefined-behaviour
  sanitizers.
* The conditions tests/test_depth_image_gpu.py relies on hold for the chosen seeds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_image_ref as ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_map_is_the_level0_template(name):
    c = ref.case(name)
    w, h = c["w"], c["h"]
    pc0 = synth.make_pc(*c["points"], c["pyr"])[0]
    inner = c["map"][2:h - 2, 2:w - 2]
    ys, xs = np.nonzero(inner > 0)
    assert len(ys) == len(pc0["u"]) > 0
    assert np.array_equal((xs + 2).astype(np.float32), pc0["u"]) and np.array_equal((ys + 2).astype(np.float32), pc0["v"])
    assert np.array_equal(inner[ys, xs], pc0["idepth"])
    assert np.array_equal(c["I0"][ys + 2, xs + 2], pc0["color"])
    assert np.array_equal(inner[~(inner > 0)], np.full(inner.size - len(ys), -1, np.float32))


def test_border_keeps_raw_sums():
    """a lone point on a border pixel leaves new_idepth * weight there, not new_idepth; its diagonal neighbour inside is dilated and
    normalised"""
    I0 = np.full((20, 24), 100, np.float32)
    m = ref.level0_map(np.array([1]), np.array([5]), np.array([0.5], np.float32), np.array([8], np.float32), I0)
    assert m[5, 1] == np.float32(4.0)
    assert m[6, 2] == np.float32(0.5) and m[4, 2] == np.float32(0.5)      # STEP3 from (1, 5), then STEP5: 4 / 8
    assert m[6, 0] == np.float32(4.0) and m[4, 0] == np.float32(4.0)      # the same dilation in the border stays a raw sum
    assert (m > 0).sum() == 5 and (m[2:-2, 2:-2] == -1).sum() == m[2:-2, 2:-2].size - 2


def test_input_conditions():
    c = ref.input_conditions("322x242")
    print(c)
    assert c["outcomes"] == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8]       # both clamps and icP 0..7
    assert c["circles_without_centre"] >= 2000                  # the nid >= 3 arm
    assert c["border_positive"] >= 200                          # raw sums the sort counts
    c = ref.input_conditions("96x64")
    print(c)
    assert c["levels"] == 2 and c["border_positive"] >= 50
    used = ref.case("96x64")["plot"]["used"]
    inner_max = ref.case("96x64")["map"][2:-2, 2:-2].max()
    assert used[1] > inner_max                                  # the raw sums take the 95th percentile
    c = ref.input_conditions("640x480")
    print(c)
    assert c["positive"] >= 80000 and c["outcomes"] == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8]


def test_scatter_order_by_hand():
    """two sources three pixels apart: the overlap shows the later one in raster order"""
    I0 = np.zeros((16, 20), np.float32)
    m = np.full((16, 20), -1, np.float32)
    m[7, 6], m[7, 9] = 0.2, 0.9                                  # jet: 0.2 -> clamp low (128, 0, 0) with range (0.5, 0.8); 0.9 -> (0, 0, 128)
    d = ref.draw(m, I0, 0.5, 0.8)
    assert d["circles"] == 2
    assert tuple(d["rgb"][7, 3]) == (128, 0, 0) and tuple(d["rgb"][7, 12]) == (0, 0, 128)
    assert tuple(d["rgb"][7, 9]) == (128, 0, 0)                 # ring of (6, 7) at dx = +3; (9, 7) does not write its own centre
    assert tuple(d["rgb"][7, 6]) == (0, 0, 128)                 # ring of (9, 7) at dx = -3
    assert tuple(d["rgb"][5, 8]) == (0, 0, 128)                 # both rings cover it: the later source wins
    assert tuple(d["rgb"][7, 7]) == (0, 0, 128) and tuple(d["rgb"][7, 8]) == (128, 0, 0)   # (7,7): dx=+1 of the first (inner), dx=-2 of the second


@pytest.mark.skipif(CXX is None, reason="g++ not found")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_depth_image_program(tmp_path, flags):
    exe = str(tmp_path / "test_depth_image")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(CSRC, "test_depth_image.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "depth_image ok" in r.stdout
