"""Call time of sdso_ingest_frame for a KITTI-shaped 8-bit stereo pair (I) against yardstick F, one process, alternating.

  F: what the library offered before once the host has already paid for the undistortion: two sdso_make_pyramid calls from ready float
     images (each ends in a stream synchronise)
  I: sdso_ingest_frame(left, right) + sdso_ctx_sync, raw 1241x376 uint8 in, mode 2 (G and vignette), RadTan crop remap to 1232x368
  C: the undistortion the host pays before F: tools/undistort_cpu_baseline.cpp, g++ -O3, one thread, the same inputs (reported apart)
Host clock around the calls, median of --reps.  A second loop with in-library profiling on gives the level-0 kernel's own time
("k_ingest_level0", HIP events tied to the dispatch) and its share of the HBM peak on algorithmic bytes.  Before timing, the two paths
are compared: the slots I fills hold the bits of the slots F fills.

  python tools/time_ingest.py [--reps 200] [--warmup 20] [--only-i]
--only-i is for a run under `rocprofv3 --kernel-trace --stats -- python tools/time_ingest.py --only-i`: the kernels alone."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi            # noqa: E402
import ingest_cases as Cs           # noqa: E402
import undistort_ref as R           # noqa: E402

HBM_PEAK = 8.0e12                   # bytes / s, the specified peak of the MI355X's HBM3E
CALIB = 3


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return "median %7.1f   p10 %7.1f   p90 %7.1f   min %7.1f  (us, n=%d)" % (np.median(t), t[len(t) // 10], t[(9 * len(t)) // 10], t[0], len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-i", action="store_true")
    args = ap.parse_args()
    size = Cs.KITTI
    wOrg, hOrg, w, h = size["wOrg"], size["hOrg"], size["w"], size["h"]
    raws = [Cs.raw_image(wOrg, hOrg, 8, 100 + i) for i in range(2)]
    G, vinv = Cs.response(8), Cs.vignette_inv(wOrg, hOrg)
    _, rx, ry, _ = R.make_remap(R.RADTAN, Cs.pars(R.RADTAN, size), wOrg, hOrg, w, h, R.CROP)
    exposure = np.array([0.011, 0.013], np.float32)
    imgs = [np.ascontiguousarray(R.undistort(raws[i], rx, ry, G, vinv, 2, exposure[i])[0]) for i in range(2)]

    ctx = abi.Context(0)
    assert Cs.calib_create(ctx, CALIB, size, (rx, ry), 8, G, vinv, 2) == 0
    ptrs = (C.c_void_p * 2)(*[r.ctypes.data for r in raws])
    slots_i, slots_f = (C.c_int * 2)(41, 42), (43, 44)

    def run_f():
        for i in range(2):
            ctx.L.sdso_make_pyramid(ctx.h, slots_f[i], w, h, abi.fp(imgs[i]))

    def run_i():
        rc = ctx.L.sdso_ingest_frame(ctx.h, CALIB, 2, slots_i, ptrs, abi.fp(exposure), 1.0, None)
        ctx.L.sdso_ctx_sync(ctx.h)
        return rc

    ctx.check(run_i())
    run_f()
    for i in range(2):
        assert Cs.same_bits(Cs.download_pyramid(ctx, slots_i[i], w, h), Cs.download_pyramid(ctx, slots_f[i], w, h)), "I and F differ"
    print("I and F hold the same bits in every level of both eyes")

    tF, tI = [], []
    for rep in range(args.warmup + args.reps):
        if not args.only_i:
            t0 = time.perf_counter()
            run_f()
            t1 = time.perf_counter()
            if rep >= args.warmup:
                tF.append(t1 - t0)
        t0 = time.perf_counter()
        run_i()
        t1 = time.perf_counter()
        if rep >= args.warmup:
            tI.append(t1 - t0)
    print("KITTI-shaped 8-bit stereo pair, %dx%d -> %dx%d, %d levels" % (wOrg, hOrg, w, h, ctx.L.sdso_pyramid_levels(w, h)))
    if not args.only_i:
        print("  F 2 x sdso_make_pyramid (float images ready) ", stats(tF))
    print("  I sdso_ingest_frame(pair) + sdso_ctx_sync     ", stats(tI))
    if args.only_i:
        ctx.close()
        return
    print("  I / F = %.3f" % (np.median(tI) / np.median(tF)))

    # the level-0 kernel alone
    ctx.check(ctx.L.sdso_prof_reset(ctx.h))
    ctx.check(ctx.L.sdso_prof_enable(ctx.h, 1))
    for _ in range(args.reps):
        run_i()
    ms, n = ctx.prof_read("k_ingest_level0")
    ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
    us = 1e3 * ms / n
    # algorithmic bytes per eye: the raw image once, the vignette once, the remap pair and the float4 pixel per output pixel (G: 1 KB)
    nbytes = 2 * (wOrg * hOrg * (1 + 4) + w * h * (8 + 16)) + 1024
    print("  k_ingest_level0: %.2f us per launch (both eyes, %d launches); %.2f MB algorithmic -> %.2f TB/s = %.1f %% of the %.1f TB/s HBM peak"
          % (us, n, nbytes / 1e6, nbytes / us / 1e6, 100.0 * nbytes / (us * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    ctx.close()

    # the CPU undistortion that precedes F in the parent path
    exe = os.path.join(ROOT, "tools", "undistort_cpu_baseline.bin")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "undistort_cpu_baseline.cpp")])
    with tempfile.TemporaryDirectory() as d:
        arrays = dict(meta=np.array([wOrg, hOrg, w, h], np.int32), raw0=raws[0], raw1=raws[1], G=G, vinv=vinv, remapX=rx, remapY=ry)
        for k, arr in arrays.items():
            np.ascontiguousarray(arr).tofile(os.path.join(d, k + ".bin"))
        cpu = json.loads(subprocess.check_output([exe, d, str(args.reps)], text=True))
    want = float(np.sum(imgs[0].astype(np.float64)) + np.sum(imgs[1].astype(np.float64)))
    assert abs(cpu["checksum"] - want) <= 1e-3 * want, (cpu["checksum"], want)
    print("  C CPU undistort of the pair (1 thread, -O3)    median %7.1f   p90 %7.1f   min %7.1f  (us, n=%d)" % (cpu["median_us"], cpu["p90_us"], cpu["min_us"], args.reps))
    print("  parent path C + F = %.1f us against I = %.1f us" % (cpu["median_us"] + np.median(tF) * 1e6, np.median(tI) * 1e6))


if __name__ == "__main__":
    main()
