"""The marginalisation prior HM / bM of sdso_ba_marginalize_points and the iteration that follows it: distance of the device and of the float
oracle from the f64-accumulator truth, one line per (window, flag pattern) of tests/marg_prior_cases.py — the numbers the docstrings of
tests/test_marg_prior_gpu.py quote.  The bars of that test come from the float oracle's columns alone.
  python tests/diag/marg_prior_errors.py > profiles/marg_prior_errors.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi  # noqa: E402
import pyoracle  # noqa: E402
import marg_prior_cases as MP  # noqa: E402


def rng(v):
    v = [x for x in v if x > 0]
    return "%.1e..%.1e (median %.1e)" % (min(v), max(v), float(np.median(v))) if v else "0"


if __name__ == "__main__":
    oracle = pyoracle.load()
    ctx = abi.Context(0)
    E_H, E_b = MP.bars(oracle)
    fb = MP.follow_bars(oracle)
    print("bars from the float oracle: 2 E_H = %.3e, 2 E_b = %.3e (the bar of tests/test_ba_marg_gpu.py: 1e-4)" % (2 * E_H, 2 * E_b))
    print("following iteration, float oracle max / median: " + ", ".join("%s %.2e / %.2e" % (k, fb[k][0], fb[k][1]) for k in fb))
    cols = {k: ([], []) for k in ("e_H", "e_b", "H", "b", "x", "step")}
    sec = {}
    for case in MP.CASES:
        win = MP.window(case)
        for pattern in MP.PATTERNS:
            f32, f64 = MP.reference(oracle, case, pattern)
            follow = "follow" in f32
            g = MP.device_marginalize(ctx, win, MP.flags(win, pattern), follow=follow)
            eg = dict(e_H=MP.e_H(g["HM"], f64["HM"]), e_b=MP.e_b(g["bM"], f64["HM"], f64["bM"]))
            line = "%-16s %-7s flagged %3d resInM %4d | e_H device %.2e oracle_f32 %.2e | e_b device %.2e oracle_f32 %.2e" % (
                case, pattern, int(MP.flags(win, pattern).sum()), g["resInM"], eg["e_H"], f32["e_H"], eg["e_b"], f32["e_b"])
            for k in ("e_H", "e_b"):
                cols[k][0].append(eg[k]); cols[k][1].append(f32[k])
            sg, _ = MP.section_errors(g["acc"], f64["acc"], win["nf"])
            so, _ = MP.section_errors(f32["acc"], f64["acc"], win["nf"])
            for (name, e, ok), (_, eo, _) in zip(sg, so):
                sec.setdefault(name, ([], []))
                sec[name][0].append(e); sec[name][1].append(eo)
                assert ok, (case, pattern, name)
            if follow:
                fg = MP.follow_distances(g, f64)
                line += " | next iteration: " + ", ".join("%s device %.2e oracle_f32 %.2e" % (k, fg[k], f32["follow"][k]) for k in fb)
                line += " | device meets H 1e-7: %s, x 1e-5: %s" % (fg["H"] <= 1e-7, fg["x"] <= 1e-5)
                for k in fb:
                    cols[k][0].append(fg[k]); cols[k][1].append(f32["follow"][k])
            print(line, flush=True)
    for k, (d, o) in cols.items():
        print("%-5s device %s | oracle_f32 %s" % (k, rng(d), rng(o)))
    for name, (d, o) in sec.items():
        print("accumulators of the marginalisation pass, %-5s device %s | oracle_f32 %s" % (name, rng(d), rng(o)))
    oE_H, oE_b = MP.orth_bars(oracle)
    print("orthogonalised (host0): bars 2 E_H = %.3e, 2 E_b = %.3e" % (2 * oE_H, 2 * oE_b))
    for case in MP.ORTH_CASES:
        for bits in MP.ORTH_BITS:
            win = MP.with_solver_bits(MP.window(case), bits)
            f32, f64 = MP.reference(oracle, case, "host0", bits)
            g = MP.device_marginalize(ctx, win, MP.flags(win, "host0"))
            print("%-16s bits %2d | e_H device %.2e oracle_f32 %.2e | e_b device %.2e oracle_f32 %.2e" % (
                case, bits, MP.e_H(g["HM"], f64["HM"]), f32["e_H"], MP.e_b(g["bM"], f64["HM"], f64["bM"]), f32["e_b"]), flush=True)
    for case in MP.ADD_CASES:
        win = MP.window(case)
        defect_o, H64 = MP.additivity_reference(oracle, case)
        HA, HB, HU = [MP.device_marginalize(ctx, win, f, want_acc=False)["HM"] for f in MP.additivity_flags(win)]
        print("%-16s additivity defect HM(A u B) - HM(A) - HM(B), whitened: device %.2e oracle_f32 %.2e" % (case, MP.whitened_defect(HU, HA, HB, H64), defect_o), flush=True)
    ctx.close()
