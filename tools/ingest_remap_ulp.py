#!/usr/bin/env python3
"""How far may a libm move the remap tables?  Evaluates tests/undistort_ref.py twice on every case of tests/ingest_cases.py — transcendental
calls in float32, and in float64 rounded to float32 — and prints the largest difference in K and in the remap entries valid on both
sides, and the number of validity flags that differ.  tests/test_undistort_ref.py allows the library four times the largest figure
(profiles/ingest_remap_ulp.txt holds the output).  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "stereo-dso-g2o_amd")]
import ingest_cases as Cs  # noqa: E402
import undistort_ref as R  # noqa: E402


def main():
    worst = 0.0
    print("%-28s %12s %12s %10s %10s" % ("case", "max|dK|", "max|dremap|", "flags", "pixels"))
    for name, model, size, mode, oc in Cs.remap_cases():
        a = R.make_remap(model, Cs.pars(model, size), size["wOrg"], size["hOrg"], size["w"], size["h"], mode, oc, "f32")
        b = R.make_remap(model, Cs.pars(model, size), size["wOrg"], size["hOrg"], size["w"], size["h"], mode, oc, "f64")
        both = (a[1] >= 0) & (b[1] >= 0)
        dk = float(np.abs(a[0] - b[0]).max())
        dr = float(max(np.abs(a[1] - b[1])[both].max(), np.abs(a[2] - b[2])[both].max()))
        flags = int(((a[1] < 0) != (b[1] < 0)).sum())
        worst = max(worst, dk, dr)
        print("%-28s %12.6g %12.6g %10d %10d" % (name, dk, dr, flags, both.size))
    print("largest difference: %.9g pixels (one ulp of a float32 coordinate in [1024, 2048) is %.9g)" % (worst, 2.0 ** -13))
    print("numpy %s" % np.__version__)


if __name__ == "__main__":
    main()
