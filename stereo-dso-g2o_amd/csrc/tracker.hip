// Coarse tracker on gfx950: fused CoarseTracker::calcRes + calcGSSSE (one launch per evaluation,
// any number of independent problems per launch) and the DSO-native LM driver of
// CoarseTracker::trackNewestCoarse.
//
// Reference (paths under /root/reference):
//   src/FullSystem/CoarseTracker.cpp:600-792  calcRes   (native body preserved as comments :699-775)
//   src/FullSystem/CoarseTracker.cpp:537-596  calcGSSSE (Accumulator9: MatrixAccumulators.h:907-1277)
//   src/FullSystem/CoarseTracker.cpp:827-1069 trackNewestCoarse (native LM preserved as comments)
//
// Kernel design (HBM/latency bound, ~160 flop for 64 algorithmic bytes per point):
//   * template points are float4 {u,v,idepth,color}: one 16-B coalesced load per lane;
//   * images are float4 {I,dx,dy,0}: the four bilinear taps are two 32-B row segments;
//   * every lane keeps the 45 upper-triangle sums of the 9x9 system + energy/statistics in
//     registers over its grid-stride loop, then a 64-lane butterfly + LDS cross-wave reduce writes
//     ONE partial record per workgroup (no atomics, deterministic);
//   * a second tiny kernel folds the partials of each problem in fixed order and applies the
//     1/n + SCALE_* scaling in double;
//   * workgroup -> (problem, chunk) mapping keeps all chunks of a problem on one XCD
//     (linear id % 8), so the problem's image rows are fetched into one L2 only.
// Per-point arithmetic is written in the reference's operation order and compiled without FP
// contraction, so residuals/Jacobian rows/inlier decisions are bit-identical to the CPU path;
// only the order of the cross-point sums differs (float tolerance, tests/test_tracker_gpu.py).
//
// One translation unit, in this order:
//   tracker_eval.hip      constants, TrackProb / TrackOut / TrackBatch, the LMS stamp macros, track_accumulate, k_track_eval,
//                         k_track_finalize, fill_eval
//   tracker_eval_api.hip  sdso_track_make_eval, sdso_track_set_ref / release_ref, the batch and single evaluation calls
//   tracker_lm_core.h     LmCore — the LM state machine of trackNewestCoarse, one text for host and device — LmJob, LM_BLOCK / LM_UNROLL
//   tracker_lm.hip        the LM step on one wave (lm_wave_ldlt, lm_exp_se3_wave, lm_wave_step), LmCluster, k_track_lm
//   tracker_lm_api.hip    resolve_job, the lock-step host driver, sdso_track_newest_coarse(_batch)
//   tracker_tries.hip     the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511): track_tries.h — the loop's rules over
//                         event traces, plain C++ — sdso_track_tries_replay, sdso_track_new_coarse
// The rules the tracker shares with g2o_factors.hip (the template level + image level lookup, the coarsestLvl range) are in
// sdso_internal.h; the sdso_se3_t <-> Se3 conversion is in host_math.h.
#include "sdso_internal.h"
#include "host_math.h"
#include <cmath>
#include <cstring>

using namespace sdso;

#include "tracker_eval.hip"
#include "tracker_eval_api.hip"
#include "tracker_lm_core.h"
#include "tracker_lm.hip"
#include "tracker_lm_api.hip"
#include "tracker_tries.hip"
