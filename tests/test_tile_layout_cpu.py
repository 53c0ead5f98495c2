"""The tiled level-0 image of the BA linearisation (csrc/tile0_layout.h: 12-byte pixels in 5x2 tiles, one 128-byte line per tile),
checked on the host: a few lines of C++ are compiled against the layout header with hipcc (host side only, no GPU needed) and walk

  * every image size w = 1..64, h = 1..9: the byte offsets of all pixels are distinct, every 12-byte pixel lies inside one 128-byte
    line, matches the formula of the layout written out with the integer operators, and the largest offset + 12 is within
    tile0_bytes(w, h) — the very function ensure_tiled0 allocates with and the window upload checks;
  * the multiply-shift division: tile0_div5 / tile0_mod5 equal x / 5 and x % 5 for every x up to TILE0_MAX_W, the widest image whose
    tiled copy the window upload accepts (and at the top of the 32-bit range, for which the header claims exactness).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-dso-g2o_amd", "csrc")

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

PROGRAM = r"""
#include "tile0_layout.h"
#include <cstdio>
#include <set>
using namespace sdso;
int main(int argc, char** argv) {
  const bool div_only = argc > 1 && argv[1][0] == 'd';
  long bad = 0;
  if (div_only) {
    for (unsigned x = 0; x <= (unsigned)TILE0_MAX_W; x++)
      if (tile0_div5(x) != x / 5u || tile0_mod5(x) != x % 5u) { if (!bad) printf("div5 wrong at %u\n", x); bad++; }
    for (unsigned x = 0xffffffffu; x > 0xffffffffu - 1000000u; x--)
      if (tile0_div5(x) != x / 5u || tile0_mod5(x) != x % 5u) { if (!bad) printf("div5 wrong at %u\n", x); bad++; }
    printf("max_w %d div_bad %ld\n", TILE0_MAX_W, bad);
    return bad != 0;
  }
  long sizes = 0;
  for (int w = 1; w <= 64; w++)
    for (int h = 1; h <= 9; h++) {
      const int T = tile0_tiles_per_row(w);
      const size_t bytes = tile0_bytes(w, h);
      if (T != (w + 4) / 5 || bytes != (size_t)128 * T * ((h + 1) / 2)) { printf("size wrong at %d x %d\n", w, h); bad++; }
      std::set<unsigned> seen;
      unsigned top = 0;
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
          const unsigned o = tile0_offset(x, y, T);
          const unsigned want = (unsigned)(((y >> 1) * T + x / 5) * 128 + (y & 1) * 60 + (x % 5) * 12);
          if (o != want) { printf("offset differs from the layout at %d x %d (%d, %d): %u, want %u\n", w, h, x, y, o, want); bad++; }
          if (!seen.insert(o).second) { printf("offset twice at %d x %d (%d, %d)\n", w, h, x, y); bad++; }
          if (o / 128 != (o + 11) / 128 || o % 4 != 0) { printf("pixel crosses a line at %d x %d (%d, %d)\n", w, h, x, y); bad++; }
          if (o % 128 >= 120) { printf("pixel in the pad at %d x %d (%d, %d)\n", w, h, x, y); bad++; }
          if (o + 12 > top) top = o + 12;
        }
      if ((size_t)top > bytes) { printf("offset %u beyond the allocation %zu at %d x %d\n", top, bytes, w, h); bad++; }
      sizes++;
    }
  printf("sizes %ld layout_bad %ld\n", sizes, bad);
  return bad != 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile0")
    src, exe = str(d / "tile0_check.hip"), str(d / "tile0_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    return r


def test_offsets_distinct_inside_lines_and_inside_the_allocation(program):
    r = _run(program)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "sizes 576 layout_bad 0" in r.stdout


def test_multiply_shift_division_is_exact_up_to_the_widest_image(program):
    r = _run(program, "d")
    assert r.returncode == 0, r.stdout[-2000:]
    assert "max_w 20971515 div_bad 0" in r.stdout
