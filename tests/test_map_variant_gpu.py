"""The A/B variant sdso_map_cloud keeps behind the debug gate (csrc/sdso_internal.h::dbg_env), through the tests of its path in a
subprocess, as tests/test_variants_gpu.py does for the others:
  SDSO_MAP_ONE_WAIT=1   the per-list counts and both arrays at their upper bound copied behind ONE wait, the used prefix handed on from
                        pinned memory, instead of a wait for the counts and a second one for the used prefix (the default;
                        tools/time_map_cloud.py times the two against each other, profiles/map_cloud_timing.txt)
The caller sees the same bytes, and nothing past the used prefix is written, either way."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_wait_variant_passes_the_cloud_tests():
    e = dict(os.environ, SDSO_MAP_ONE_WAIT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_map_gpu.py", "-k",
                        "hand_made or world_frame or repeatable or cloud_refusals or camera_frame_cloud"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1500:])
    assert " passed" in r.stdout
