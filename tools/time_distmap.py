"""Times sdso_distmap_make and sdso_activate_select (1232x368, ~2 000 seeds, 14 000 candidates; also the dense and sparse regimes of
tests/distmap_cases.py) on the GPU, next to a single-thread -O3 C++ restatement of the same two steps on the same host
(tools/distmap_cpu_baseline.cpp, built here).  Warm-up, then repeated calls: wall time of the whole call including the copies with the
in-library profiling off, kernel times from HIP events (sdso_prof_*) in a loop of their own.  Prints the report; profiles/distmap_timing.txt
is this output."""
import ctypes as C, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("stereo-dso-g2o_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
from sdso_amd import abi
import distmap_cases as Cs

WARM, REPS = 5, 50
exe = os.path.join(ROOT, "tools", "distmap_cpu_baseline.bin")
subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "distmap_cpu_baseline.cpp")])
ctx = abi.Context(0)
print("distance map + activation candidate selection, %d warm-up + %d timed calls each; times in microseconds (median / min)" % (WARM, REPS))
for name in sorted(Cs.REGIMES):
    case = Cs.selection_case(**Cs.REGIMES[name])
    a, c = case["active"], case["cand"]
    w, h, n = case["w"], case["h"], len(case["cand"]["u"])
    G = abi.make_distmap_geoms(case["KRKi"], case["Kt"])
    flagged = np.ascontiguousarray(case["flagged"], np.uint8)
    S = abi.ActivateSelect()
    S.w, S.h, S.ngeom, S.n = w, h, len(case["KRKi"]), n
    S.geom = C.cast(G, C.POINTER(abi.DistMapGeom)); S.host_flagged = abi.bp(flagged)
    S.point_geom = abi.ip(c["pg"]); S.u = abi.fp(c["u"]); S.v = abi.fp(c["v"]); S.idepth_min = abi.fp(c["idepth_min"]); S.idepth_max = abi.fp(c["idepth_max"])
    S.quality = abi.fp(c["quality"]); S.lastTracePixelInterval = abi.fp(c["interval"]); S.lastTraceStatus = abi.bp(c["status"]); S.my_type = abi.fp(c["my_type"])
    S.currentMinActDist = float(case["min_act_dist"]); S.minTraceQuality = float(case["min_trace_quality"])
    dec, iu, iv, nsel, ns = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int(0), C.c_int(0)

    def loop(prof):
        """make + select, WARM + REPS times; the wall times of the two calls (each ends in a stream synchronise)"""
        ctx.check(ctx.L.sdso_prof_reset(ctx.h)); ctx.check(ctx.L.sdso_prof_enable(ctx.h, prof))
        tm, ts = [], []
        for i in range(WARM + REPS):
            t0 = time.perf_counter()
            ctx.check(ctx.L.sdso_distmap_make(ctx.h, w, h, len(case["KRKi"]), G, len(a["u"]), abi.ip(a["pg"]), abi.fp(a["u"]), abi.fp(a["v"]), abi.fp(a["idepth"]), C.byref(ns)))
            t1 = time.perf_counter()
            ctx.check(ctx.L.sdso_activate_select(ctx.h, C.byref(S), abi.bp(dec), abi.ip(iu), abi.ip(iv), C.byref(nsel)))
            t2 = time.perf_counter()
            if i >= WARM:
                tm.append((t1 - t0) * 1e6); ts.append((t2 - t1) * 1e6)
        return tm, ts
    tm, ts = loop(0)
    loop(2)
    kern = {}
    for k in ("k_distmap_seed", "k_distmap_grow", "k_select_classify", "k_distmap_select"):
        ms, cnt = ctx.prof_read(k)
        kern[k] = ms * 1e3 / max(cnt, 1)
    ctx.check(ctx.L.sdso_prof_enable(ctx.h, 0))
    final = Cs.dm_get(ctx, w, h)
    # ---- the CPU restatement on the same inputs
    with tempfile.TemporaryDirectory() as d:
        arrays = dict(meta=np.array([w, h], np.int32), geom=np.concatenate([case["KRKi"].reshape(-1, 9), case["Kt"].reshape(-1, 3)], axis=1).astype(np.float32),
                      flagged=flagged, a_pg=a["pg"], a_u=a["u"], a_v=a["v"], a_idepth=a["idepth"], c_pg=c["pg"], c_status=c["status"], c_u=c["u"], c_v=c["v"],
                      c_idepth_min=c["idepth_min"], c_idepth_max=c["idepth_max"], c_quality=c["quality"], c_interval=c["interval"], c_my_type=c["my_type"],
                      par=np.array([case["min_act_dist"], case["min_trace_quality"]], np.float32))
        for k, arr in arrays.items():
            np.ascontiguousarray(arr).tofile(os.path.join(d, k + ".bin"))
        cpu = json.loads(subprocess.check_output([exe, d, str(REPS)], text=True))
    agree = cpu["n_seeds"] == ns.value and cpu["n_selected"] == nsel.value and cpu["final_map_sum"] == float(final.astype(np.float64).sum())
    print("\n%s: %dx%d, currentMinActDist %.1f, %d active points -> %d seeds, %d candidates -> %d selected (CPU restatement agrees: %s)"
          % (name, w, h, float(case["min_act_dist"]), len(a["u"]), ns.value, n, nsel.value, agree))
    print("  sdso_distmap_make     all-in %8.1f / %8.1f   kernels: k_distmap_seed %.1f + k_distmap_grow %.1f     CPU -O3 single thread %8.1f / %8.1f"
          % (np.median(tm), min(tm), kern["k_distmap_seed"], kern["k_distmap_grow"], cpu["make_us_median"], cpu["make_us_min"]))
    print("  sdso_activate_select  all-in %8.1f / %8.1f   kernels: k_select_classify %.1f + k_distmap_select %.1f   CPU -O3 single thread %8.1f / %8.1f"
          % (np.median(ts), min(ts), kern["k_select_classify"], kern["k_distmap_select"], cpu["select_us_median"], cpu["select_us_min"]))
    print("  k_distmap_select per selected candidate: %.2f us" % (kern["k_distmap_select"] / max(nsel.value, 1)))
ctx.close()
