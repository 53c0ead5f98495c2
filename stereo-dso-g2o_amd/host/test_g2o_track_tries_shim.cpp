// sdso_shim::CoarseTracker::trackNewCoarse with forkLive = true — FullSystem::trackNewCoarse STEP2-4 (FullSystem.cpp:436-511) around the
// fork's live trackNewestCoarse — driven on the stand-in types the way the reference's body would drive it: a FrameHessian, a
// std::vector<SE3> of tries, AffLight, Vec5 lastCoarseRMSE by reference.  tests/test_g2o_track_tries_shim_gpu.py writes one tracking problem
// and several try lists, runs this program and compares what it dumps with the same lists pushed through sdso_g2o_track_new_coarse from
// Python.  The arrays are those of test_track_tries_shim.cpp.
//
//   test_g2o_track_tries_shim <dir>
// in:  meta (levels w0 h0 coarsestLvl nlists), calib (fx fy cx cy), misc (ref_exposure new_exposure ref_a ref_b reTrackThreshold),
//      ref_l<l> / new_l<l>, pc_{u,v,idepth,color}_l<l>, ntries (per list), tries (12 doubles per try, all lists), aff0 (2 per list),
//      rmse (5 per list)
// out: ints (per list: haveOneGood winner tryIterations), doubles (per list: pose 12, aff 2, flowVecs 3, achievedRes 5, lastCoarseRMSE 5,
//      lastResiduals 5, lastFlowIndicators 3, firstCoarseRMSE), per_try (per try: ran good abort_lvl winner)
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_g2o_track_tries_shim <dir>\n"); return 2; }
  try {
    const std::string dir = argv[1];
    auto meta = load<int>(dir, "meta");
    auto calib = load<double>(dir, "calib");
    auto misc = load<double>(dir, "misc");
    const int levels = meta[0], w0 = meta[1], h0 = meta[2], coarsestLvl = meta[3], nlists = meta[4];
    sdso_shim::Device dev(0);
    FrameHessian ref, cur;
    load_pyramid(dir, "ref", ref, levels); load_pyramid(dir, "new", cur, levels);
    ref.slot = 0; cur.slot = 1;
    cur.ab_exposure = (float)misc[1];
    int w[SDSO_PYR_LEVELS], h[SDSO_PYR_LEVELS];
    for (int l = 0; l < levels; l++) { w[l] = w0 >> l; h[l] = h0 >> l; }
    dev.uploadFrame(ref.slot, &ref, levels, w, h); dev.uploadFrame(cur.slot, &cur, levels, w, h);
    CalibHessian HC; for (int i = 0; i < 4; i++) HC.value_scaled[i] = HC.value_zero[i] = calib[i];
    sdso_shim::CoarseTracker<SE3, AffLight, Mat33, Vec3> tracker(dev, 0);
    tracker.forkLive = true;
    tracker.makeK(&HC, levels, w0, h0);
    tracker.slot_of = [](const void* fh) { return static_cast<const FrameHessian*>(fh)->slot; };
    AffLight refAff; refAff.a = misc[2]; refAff.b = misc[3];
    for (int l = 0; l < levels; l++) {
      const std::string s = "_l" + std::to_string(l);
      auto pu = load<float>(dir, "pc_u" + s), pv = load<float>(dir, "pc_v" + s), pi = load<float>(dir, "pc_idepth" + s), pc = load<float>(dir, "pc_color" + s);
      tracker.setCoarseTrackingRef(l, (int)pu.size(), pu.data(), pv.data(), pi.data(), pc.data(), (float)misc[0], refAff, 7);
    }
    if (tracker.firstCoarseRMSE != -1) { std::fprintf(stderr, "firstCoarseRMSE after a new reference\n"); return 1; }
    auto ntries = load<int>(dir, "ntries");
    auto tr = load<double>(dir, "tries"), aff0 = load<double>(dir, "aff0"), rmse = load<double>(dir, "rmse");
    std::vector<int> o_int, o_try;
    std::vector<double> o_dbl;
    size_t t0 = 0;
    for (int k = 0; k < nlists; k++) {
      std::vector<SE3> lastF_2_fh_tries;
      for (int i = 0; i < ntries[k]; i++) lastF_2_fh_tries.push_back(se3_of(&tr[(t0 + i) * 12]));
      t0 += ntries[k];
      AffLight aff_last_2_l; aff_last_2_l.a = aff0[k * 2]; aff_last_2_l.b = aff0[k * 2 + 1];
      Vec5 lastCoarseRMSE, achievedRes;
      for (int i = 0; i < 5; i++) lastCoarseRMSE[i] = rmse[k * 5 + i];
      Vec3 flowVecs; for (int i = 0; i < 3; i++) flowVecs[i] = 100;      // FullSystem.cpp:425
      SE3 lastF_2_fh;
      AffLight aff_g2l;
      int tryIterations = 0;
      const bool haveOneGood = tracker.trackNewCoarse(&cur, lastF_2_fh_tries, aff_last_2_l, coarsestLvl, lastCoarseRMSE, (float)misc[4], lastF_2_fh, aff_g2l,
                                                      flowVecs, achievedRes, tryIterations);
      o_int.push_back(haveOneGood ? 1 : 0); o_int.push_back(tracker.lastTriesResult.winner); o_int.push_back(tryIterations);
      for (int i = 0; i < 9; i++) o_dbl.push_back(lastF_2_fh.R.m[i]);
      for (int i = 0; i < 3; i++) o_dbl.push_back(lastF_2_fh.t[i]);
      o_dbl.push_back(aff_g2l.a); o_dbl.push_back(aff_g2l.b);
      for (int i = 0; i < 3; i++) o_dbl.push_back(flowVecs[i]);
      for (int i = 0; i < 5; i++) o_dbl.push_back(achievedRes[i]);
      for (int i = 0; i < 5; i++) o_dbl.push_back(lastCoarseRMSE[i]);
      for (int i = 0; i < 5; i++) o_dbl.push_back(tracker.lastResiduals[i]);
      for (int i = 0; i < 3; i++) o_dbl.push_back(tracker.lastFlowIndicators[i]);
      o_dbl.push_back(tracker.firstCoarseRMSE);
      for (const sdso_track_try_t& r : tracker.lastTries) { o_try.push_back(r.ran); o_try.push_back(r.good); o_try.push_back(r.abort_lvl); o_try.push_back(r.winner); }
    }
    dump(dir, "ints", o_int); dump(dir, "doubles", o_dbl); dump(dir, "per_try", o_try);
    std::printf("g2o_track_tries_shim ok: %d lists\n", nlists);
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
