// The loop over the motion tries of FullSystem::trackNewCoarse as a state machine over EVENT TRACES, stated once: sdso_track_new_coarse and
// sdso_track_tries_replay (tracker_tries.hip) walk it, csrc/test_track_tries.cpp checks it on a CPU.  Plain C++, no HIP type, no ctx.
//
// Reference:
//   src/FullSystem/FullSystem.cpp:436-511       the loop: achievedRes, the winner, the carry, the stop, the no-good-try ending
//   src/FullSystem/CoarseTracker.cpp:855-856    a call resets lastResiduals to NaN and lastFlowIndicators to 1000
//   src/FullSystem/CoarseTracker.cpp:1029-1040  a level ends: lastResiduals[lvl], lastFlowIndicators, the abort test, the repetition
// A try is given by what it produced when it ran under bounds no tighter than the loop's (the `in` members of sdso_track_try_t): the
// residual and the flow indicators of every finish_level event (LmCore::finish_level, tracker_lm_core.h) and what it ends with if no
// abort fires.  The abort test is replayed per event against the loop's own bounds — also on the first pass of a repeated level, whose
// residual the second pass overwrites.
#pragma once
#include <cmath>
#include "../../include/sdso_abi.h"

namespace sdso {

struct TrackTries {
  double achievedRes[5];       // :436
  int haveOneGood = 0;         // :437
  int winner = -1;
  int tryIterations = 0;       // :438
  double flowVecs[3];          // :425
  sdso_se3_t pose;             // lastF_2_fh (:428)
  sdso_aff_t aff;              // aff_g2l (:430)

  void init() {
    for (int i = 0; i < 5; i++) achievedRes[i] = NAN;
    haveOneGood = 0; winner = -1; tryIterations = 0;
    for (int i = 0; i < 3; i++) flowVecs[i] = 100;
    for (int i = 0; i < 9; i++) pose.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; i++) pose.t[i] = 0;
    aff.a = 0; aff.b = 0;
  }

  // what trackNewestCoarse leaves when it runs the try `r` under minResForAbort = achievedRes (:445-449): fills r's `out` members
  // besides `winner`
  void see(const sdso_se3_t& try_pose, const sdso_aff_t& aff_last_2_l, sdso_track_try_t& r) const {
    r.ran = 1; r.abort_lvl = -1; r.winner = 0;
    for (int i = 0; i < 5; i++) r.lastResiduals[i] = NAN;           // CoarseTracker.cpp:855
    for (int i = 0; i < 3; i++) r.lastFlowIndicators[i] = 1000;     // :856
    for (int e = 0; e < r.trace.n; e++) {
      const int lvl = r.trace.lvl[e];
      r.lastResiduals[lvl] = r.trace.res[e];                        // :1029
      for (int i = 0; i < 3; i++) r.lastFlowIndicators[i] = r.trace.flow[e][i];   // :1030
      if (r.lastResiduals[lvl] > 1.5 * achievedRes[lvl]) { r.abort_lvl = lvl; break; }   // :1032 (false for a NaN bound)
    }
    if (r.abort_lvl >= 0) { r.good = 0; r.pose = try_pose; r.aff = aff_last_2_l; }   // return false before :1044: the references stay untouched
    else { r.good = r.end_good; r.pose = r.end_pose; r.aff = r.end_aff; }
  }

  // one trip of the loop (:441-501) on try i; returns true where the loop breaks (:499-500)
  bool step(int i, const sdso_se3_t& try_pose, const sdso_aff_t& aff_last_2_l, double lastCoarseRMSE0, double reTrackThreshold, sdso_track_try_t& r) {
    see(try_pose, aff_last_2_l, r);
    tryIterations++;                                                // :451
    if (r.good && std::isfinite((float)r.lastResiduals[0]) && !(r.lastResiduals[0] >= achievedRes[0])) {   // :475-477
      for (int k = 0; k < 3; k++) flowVecs[k] = r.lastFlowIndicators[k];
      aff = r.aff;
      pose = r.pose;
      haveOneGood = 1;
      winner = i;
      r.winner = 1;
    }
    if (haveOneGood) {                                              // :487-496
      for (int k = 0; k < 5; k++)
        if (!std::isfinite((float)achievedRes[k]) || achievedRes[k] > r.lastResiduals[k]) achievedRes[k] = r.lastResiduals[k];
    }
    return haveOneGood && achievedRes[0] < lastCoarseRMSE0 * reTrackThreshold;   // :499
  }

  // after the loop (:503-511): the ending without a good try, the result, lastCoarseRMSE = achievedRes
  void finish(const sdso_se3_t& try0, const sdso_aff_t& aff_last_2_l, double* lastCoarseRMSE, sdso_track_tries_result_t& out) {
    if (!haveOneGood) {
      for (int k = 0; k < 3; k++) flowVecs[k] = 0;
      aff = aff_last_2_l;
      pose = try0;
    }
    out.haveOneGood = haveOneGood; out.winner = winner; out.tryIterations = tryIterations;
    out.pose = pose; out.aff = aff;
    for (int k = 0; k < 3; k++) out.flowVecs[k] = flowVecs[k];
    for (int k = 0; k < 5; k++) { out.achievedRes[k] = achievedRes[k]; lastCoarseRMSE[k] = achievedRes[k]; }
  }
};

// a try the loop never reached
inline void track_try_not_run(sdso_track_try_t& r) { r.ran = 0; }

inline bool track_trace_ok(const sdso_track_trace_t& t) {
  if (t.n < 0 || t.n > SDSO_TRACK_MAX_EVENTS) return false;
  for (int e = 0; e < t.n; e++) if (t.lvl[e] < 0 || t.lvl[e] > 4) return false;
  return true;
}

// the whole loop over recs[0..ntries-1]; the caller has checked the arguments (track_trace_ok, ntries >= 1)
inline void track_tries_replay(int ntries, const sdso_se3_t* tries, const sdso_aff_t& aff_last_2_l, sdso_track_try_t* recs, double* lastCoarseRMSE,
                               double reTrackThreshold, sdso_track_tries_result_t& out) {
  TrackTries S;
  S.init();
  int i = 0;
  for (; i < ntries; i++)
    if (S.step(i, tries[i], aff_last_2_l, lastCoarseRMSE[0], reTrackThreshold, recs[i])) { i++; break; }
  for (; i < ntries; i++) track_try_not_run(recs[i]);
  S.finish(tries[0], aff_last_2_l, lastCoarseRMSE, out);
}

}  // namespace sdso
