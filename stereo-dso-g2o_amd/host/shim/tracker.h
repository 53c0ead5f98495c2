#pragma once
#include <cmath>
#include <cstring>
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
// Drop-in for the tracking half of dso::CoarseTracker.  Template parameters are the reference's own
// types; Mat33/Vec3 are the Eigen double types used to rebuild an SE3.
template <class SE3T, class AffLightT, class Mat33T, class Vec3T> class CoarseTracker {
 public:
  // publishDepthImages: the hook for debugPlotIDepthMap / debugPlotIDepthMapFloat.  FullSystem owns the wrapper list (outputWrapper) and
  // hands it to those two members per call, so the tracker cannot see at construction whether anyone listens: the caller says so here —
  // pass !outputWrapper.empty() for coarseTracker and coarseTracker_forNewKF.  true switches sdso_track_keep_depth_map on for the Device
  // (every template built on it from then on keeps its level-0 map); false leaves the library as it is and the two members throw.
  CoarseTracker(Device& dev, int ref_slot, bool publishDepthImages = false) : dev_(dev), ref_slot_(ref_slot), publish_(publishDepthImages) {
    if (publish_) dev_.check(sdso_track_keep_depth_map(dev_.ctx(), 1), "sdso_track_keep_depth_map");
    std::memset(&prm_, 0, sizeof(prm_));
    prm_.coarseCutoffTH = 20.f; prm_.huberTH = 9.f;                 // settings.cpp:102, :95
    const int its[5] = {10, 20, 50, 50, 50};                         // CoarseTracker.cpp:861 (DSO-native)
    for (int i = 0; i < 5; i++) { prm_.maxIterations[i] = its[i]; lastResiduals[i] = NAN; }
    prm_.affineOptModeA = 1e12; prm_.affineOptModeB = 1e8;            // settings.cpp:90-91
    for (int i = 0; i < 3; i++) lastFlowIndicators[i] = 1000;
  }
  // makeK(CalibHessian*): per-level intrinsics exactly as CoarseTracker.cpp:108-136
  template <class CalibHessianT> void makeK(CalibHessianT* HCalib, int pyrLevelsUsed, int w0, int h0) {
    prm_.levels = pyrLevelsUsed;
    detail::levelIntrinsics(HCalib, pyrLevelsUsed, w0, h0, prm_.w, prm_.h, prm_.fx, prm_.fy, prm_.cx, prm_.cy);
  }
  // The template point cloud the reference builds in makeCoarseDepthL0 (CoarseTracker.cpp:507-532):
  // pc_u/pc_v/pc_idepth/pc_color[lvl], pc_n[lvl].  Called once per new reference keyframe.
  void setCoarseTrackingRef(int lvl, int pc_n, const float* pc_u, const float* pc_v, const float* pc_idepth, const float* pc_color,
                            float lastRef_ab_exposure, const AffLightT& lastRef_aff_g2l_, int refFrameID_) {
    dev_.check(sdso_track_set_ref(dev_.ctx(), ref_slot_, lvl, pc_n, pc_u, pc_v, pc_idepth, pc_color), "sdso_track_set_ref");
    newRef_(nullptr, -1, refFrameID_, lastRef_ab_exposure, lastRef_aff_g2l_);   // a template from the host carries no level-0 map
  }
  // makeCoarseDepthL0 (CoarseTracker.cpp:275-534) from STEP1's per-point results: integer pixel (u,v) on lastRef, the
  // (stereo-refined) new_idepth and weight = sqrtf(1e-3 / (HdiF + 1e-12)).  Splat, pyramid, dilation, normalisation and
  // the raster-order compaction run on the device; pc_n[lvl] comes back for the reference's bookkeeping.
  void makeCoarseDepthL0(int lastRef_slot, int n, const int* u, const int* v, const float* new_idepth, const float* weight, int* pc_n,
                         float lastRef_ab_exposure, const AffLightT& lastRef_aff_g2l_, int refFrameID_) {
    dev_.check(sdso_track_make_ref(dev_.ctx(), ref_slot_, lastRef_slot, n, u, v, new_idepth, weight, pc_n), "sdso_track_make_ref");
    newRef_(nullptr, lastRef_slot, refFrameID_, lastRef_ab_exposure, lastRef_aff_g2l_);
  }
  // void setCoarseTrackingRef(std::vector<FrameHessian*> frameHessians, FrameHessian* fh_right, CalibHessian Hcalib) — CoarseTracker.h:71-72,
  // CoarseTracker.cpp:807-826 with makeCoarseDepthL0 (:275-534) entirely on the device.  STEP1 (:288-356): every point whose residual into
  // the newest keyframe is IN is re-observed by static stereo — ImmaturePoint at the rounded centerProjectedTo on fh_target, traceStereo
  // into fh_right with the interval [0.1, 1.9] * centerProjectedTo[2], and where that is IPS_GOOD back again from lastTraceUV —
  // (sdso_stereo_match_batch: ONE launch chain for all points), the accept rule of :329-341 picks idepth_stereo or centerProjectedTo[2],
  // weight = sqrtf(1e-3 / (HdiF + 1e-12)); STEP2-5 = sdso_track_make_ref.  `slot_of` maps a FrameHessian to the pyramid slot it was
  // uploaded to; `baseline` is the global of util/settings.h that traceStereo reads (ImmaturePoint.cpp:101).
  std::function<int(const void*)> slot_of;
  float baseline = 0.f;
  int pc_n[SDSO_PYR_LEVELS] = {0, 0, 0, 0, 0, 0};
  template <class FrameHessianT, class CalibHessianT>
  void setCoarseTrackingRef(std::vector<FrameHessianT*> frameHessians, FrameHessianT* fh_right, CalibHessianT Hcalib) {
    if (frameHessians.empty() || !slot_of) throw Error("setCoarseTrackingRef: no frames / slot_of not set");
    FrameHessianT* lastRef = frameHessians.back();           // (= fh_target of makeCoarseDepthL0)
    std::vector<float> fu, fv, imin, imax, cpt2, wgt;
    for (FrameHessianT* fh : frameHessians)
      for (auto* ph : fh->pointHessians) {
        if (ph->lastResiduals[0].first != 0 && (int)ph->lastResiduals[0].second == 0 /* ResState::IN */) {
          auto* r = ph->lastResiduals[0].first;
          const int u = r->centerProjectedTo[0] + 0.5f;      // :303-304
          const int v = r->centerProjectedTo[1] + 0.5f;
          fu.push_back((float)u); fv.push_back((float)v);
          imin.push_back(r->centerProjectedTo[2] * 0.1f);     // :311-312
          imax.push_back(r->centerProjectedTo[2] * 1.9f);
          cpt2.push_back(r->centerProjectedTo[2]);
          wgt.push_back(sqrtf(1e-3 / (ph->efPoint->HdiF + 1e-12)));   // :350
        }
      }
    const int n = (int)fu.size();
    std::vector<uint8_t> sf(n), sb(n);
    std::vector<float> ids(n), buv((size_t)n * 2);
    if (n) {
      sdso_stereo_match_t m;
      std::memset(&m, 0, sizeof(m));
      m.n = n; m.u = fu.data(); m.v = fv.data();
      m.idepth_min_stereo = imin.data(); m.idepth_max_stereo = imax.data();
      m.back_idepth_min_stereo = imin.data(); m.back_idepth_max_stereo = imax.data();   // :323-324
      m.status_fwd = sf.data(); m.status_back = sb.data(); m.idepth_stereo = ids.data(); m.back_uv = buv.data();
      float K4[4]; detail::calibK4(Hcalib, K4);
      dev_.check(sdso_stereo_match_batch(dev_.ctx(), slot_of(lastRef), slot_of(fh_right), K4, baseline, 1, &m), "sdso_stereo_match_batch");
    }
    std::vector<int> iu(n), iv(n);
    std::vector<float> nid(n);
    for (int i = 0; i < n; i++) {
      iu[i] = (int)fu[i]; iv[i] = (int)fv[i];
      float new_idepth = cpt2[i];
      if (sf[i] == 0 /* IPS_GOOD */) {
        const float depth = 1.0f / ids[i];
        const float u_delta = std::fabs(fu[i] - buv[(size_t)i * 2]);
        if (u_delta < 1 && depth > 0 && depth < 50) new_idepth = ids[i];            // :329-332
      }
      nid[i] = new_idepth;
    }
    installRef_(lastRef, n, iu.data(), iv.data(), nid.data(), wgt.data());
  }
  // The same member on the DEVICE-RESIDENT window of `ba` (a WindowedBA whose optimize() has just run): STEP1's walk over the pointer graph,
  // the uploads of the match batch, its download, the accept rule and the uploads of sdso_track_make_ref all stay on the device
  // (sdso_track_make_ref_from_window).  What remains here is the ORDER: STEP1 adds the points of one pixel in frameHessians[*]->pointHessians
  // order (:290-354), which differs from the window's order (EFFrame::points) once flagPointsForRemoval's compaction (FullSystem.cpp:1047-1053)
  // and removePoint's swap-with-back (EnergyFunctional.cpp:755-771) have both run — every pointHessian is looked up in the window and the
  // indices travel as point_order.  K is the window's calibration after the optimize (= Hcalib.fxl() .. cyl()), lastRef its last frame.
  // Nothing on this path reads PointFrameResidual::centerProjectedTo / projectedTo: see WindowedBA::writeBackProjections.
  int n_points = 0, n_border = 0;                            // of the latest call: points splatted; of them, too close to the border for stereo
  template <class WindowedBAT, class FrameHessianT>
  void setCoarseTrackingRef(WindowedBAT& ba, std::vector<FrameHessianT*> frameHessians, FrameHessianT* fh_right) {
    if (frameHessians.empty() || !slot_of) throw Error("setCoarseTrackingRef: no frames / slot_of not set");
    FrameHessianT* lastRef = frameHessians.back();
    std::vector<int> order;
    for (FrameHessianT* fh : frameHessians)
      for (auto* ph : fh->pointHessians) {
        const int i = ba.pointIndexOf(ph->efPoint);
        if (i < 0) throw Error("setCoarseTrackingRef: a pointHessian is not part of the device window (a point the WindowedBA was not told about?)");
        order.push_back(i);
      }
    dev_.check(sdso_track_make_ref_from_window(dev_.ctx(), ref_slot_, ba.win(), slot_of(fh_right), baseline, order.data(), (int)order.size(), &n_points,
                                               &n_border, pc_n), "sdso_track_make_ref_from_window");
    newRef_(lastRef);
  }
  // void setCTRefForFirstFrame(std::vector<FrameHessian*> frameHessians) — CoarseTracker.cpp:794-805 with makeCoarseDepthForFirstFrame
  // (:138-271): the first keyframe's own points at int(u + 0.5f), their idepth, no stereo refinement; STEP2-5 are makeCoarseDepthL0's.
  template <class FrameHessianT> void setCTRefForFirstFrame(std::vector<FrameHessianT*> frameHessians) {
    if (frameHessians.empty() || !slot_of) throw Error("setCTRefForFirstFrame: no frames / slot_of not set");
    FrameHessianT* lastRef = frameHessians.back();
    std::vector<int> iu, iv;
    std::vector<float> nid, wgt;
    for (auto* ph : lastRef->pointHessians) {
      const int u = ph->u + 0.5f;                            // :144-145
      const int v = ph->v + 0.5f;
      iu.push_back(u); iv.push_back(v); nid.push_back(ph->idepth);
      wgt.push_back(sqrtf(1e-3 / (ph->efPoint->HdiF + 1e-12)));
    }
    installRef_(lastRef, (int)iu.size(), iu.data(), iv.data(), nid.data(), wgt.data());
  }
  // The swap of FullSystem.cpp:1102-1109 between two Devices.  The reference swaps the POINTERS coarseTracker / coarseTracker_forNewKF
  // under coarseTrackerSwapMutex, after which the tracking thread calls into the object the mapping thread built; here each thread keeps
  // its own tracker on its own Device, and the template travels: makeKeyFrame ends with exportRef() on coarseTracker_forNewKF (under
  // the same mutex), the tracking thread's adoptRef() takes the place of the swap.  Device to device, no copy, no host wait.
  struct TrackingRef {
    Shared shared;                       // the template's levels
    const void* lastRef = nullptr;       // FrameHessian* of the keyframe it was built on
    int lastRef_slot = -1;               // ... and its pyramid slot ON THE BUILDER'S Device
    int refFrameID = -1;
    float ab_exposure = 0.f;
    AffLightT lastRef_aff_g2l{};
    int pc_n[SDSO_PYR_LEVELS] = {0, 0, 0, 0, 0, 0};
  };
  TrackingRef exportRef() {
    TrackingRef r;
    sdso_shared* h = nullptr;
    dev_.check(sdso_track_export_ref(dev_.ctx(), ref_slot_, &h), "sdso_track_export_ref");
    r.shared = Shared(h);
    r.lastRef = lastRef_; r.lastRef_slot = lastRef_slot_; r.refFrameID = refFrameID;
    r.ab_exposure = prm_.ref_exposure; r.lastRef_aff_g2l = lastRef_aff_g2l;
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) r.pc_n[l] = pc_n[l];
    return r;
  }
  // works on a tracker built on ANOTHER Device (of the same GPU).  The kept level-0 map stays with the builder: the two debugPlot members
  // throw on an adopting tracker as they do for a template without a map (the reference calls them on coarseTracker_forNewKF only).
  void adoptRef(const TrackingRef& r) {
    dev_.check(sdso_track_import_ref(dev_.ctx(), ref_slot_, r.shared.get()), "sdso_track_import_ref");
    lastRef_aff_g2l = r.lastRef_aff_g2l;
    newRef_(r.lastRef, r.lastRef_slot, r.refFrameID, r.ab_exposure, r.lastRef_aff_g2l);
    adopted_ = true;
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) pc_n[l] = r.pc_n[l];
  }
  // void debugPlotIDepthMap(float* minID_pt, float* maxID_pt, std::vector<IOWrap::Output3DWrapper*>& wraps) — CoarseTracker.cpp:1071-1176,
  // what FullSystem::makeKeyFrame calls on coarseTracker_forNewKF for every keyframe (FullSystem.cpp:1444).  The sort of :1078-1088, the
  // smoothing of :1094-1117 and the image of :1119-1163 run on the device on the map the latest template kept (sdso_track_depth_image);
  // here: the early return of :1072, the MinimalImageB3 the wrappers receive, and the pushes of :1167-1168.  The call also brings the
  // float map to the host, where debugPlotIDepthMapFloat finds it.  MinimalImageB3T is named by the caller: dso::MinimalImageB3.
  // (debugSaveImages' writeImage, :1170-1174, is the caller's: the image is the one the wrappers were handed.)
  template <class MinimalImageB3T, class WrapT> void debugPlotIDepthMap(float* minID_pt, float* maxID_pt, std::vector<WrapT*>& wraps) {
    if (prm_.w[1] == 0) return;                              // :1072
    requireMap_("debugPlotIDepthMap");
    const int w = prm_.w[0], h = prm_.h[0];
    MinimalImageB3T mf(w, h);
    static_assert(sizeof(*mf.data) == 3, "MinimalImageB3 holds three bytes per pixel");
    idepth0_.resize((size_t)w * h);
    float lo = minID_pt ? *minID_pt : 0.f, hi = maxID_pt ? *maxID_pt : 0.f;
    const bool both = minID_pt != 0 && maxID_pt != 0;        // :1094: otherwise the new range is used and nothing is written back
    dev_.check(sdso_track_depth_image(dev_.ctx(), ref_slot_, lastRef_slot_, both ? &lo : nullptr, both ? &hi : nullptr,
                                      reinterpret_cast<uint8_t*>(mf.data), idepth0_.data(), depthImageCounts), "sdso_track_depth_image");
    if (both) { *minID_pt = lo; *maxID_pt = hi; }
    idepth0_ok_ = true;
    for (WrapT* ow : wraps) ow->pushDepthImage(&mf);         // :1167-1168
  }
  // void debugPlotIDepthMapFloat(std::vector<IOWrap::Output3DWrapper*>& wraps) — CoarseTracker.cpp:1178-1188: a MinimalImageF that wraps
  // idepth[0] without copying, pushed with lastRef.  idepth[0] is the host copy debugPlotIDepthMap brought along (FullSystem.cpp:1444-1445
  // calls the two back to back); called on its own, the member downloads the map first.  The wrapped memory stays valid until the next
  // call of either member.  FrameHessianT is the type setCoarseTrackingRef was given (dso::FrameHessian).
  template <class MinimalImageFT, class FrameHessianT, class WrapT> void debugPlotIDepthMapFloat(std::vector<WrapT*>& wraps) {
    if (prm_.w[1] == 0) return;                              // :1179
    requireMap_("debugPlotIDepthMapFloat");
    const int w = prm_.w[0], h = prm_.h[0];
    if (!idepth0_ok_) {
      idepth0_.resize((size_t)w * h);
      dev_.check(sdso_track_depth_image(dev_.ctx(), ref_slot_, lastRef_slot_, nullptr, nullptr, nullptr, idepth0_.data(), depthImageCounts), "sdso_track_depth_image");
      idepth0_ok_ = true;
    }
    MinimalImageFT mim(w, h, idepth0_.data());               // :1183
    FrameHessianT* lastRef = static_cast<FrameHessianT*>(const_cast<void*>(lastRef_));
    for (WrapT* ow : wraps) ow->pushDepthImageFloat(&mim, lastRef);   // :1185-1187
  }
  int depthImageCounts[2] = {0, 0};                          // of the latest image: allID.size(), pixels that drew a circle
  // bool trackNewestCoarse(FrameHessian* newFrameHessian, SE3& lastToNew_out, AffLight& aff_g2l_out, int coarsestLvl, Vec5 minResForAbort,
  //                        IOWrap::Output3DWrapper* wrap = 0) — CoarseTracker.h:62-66 verbatim (the debug wrapper is not used)
  template <class FrameHessianT, class Vec5T>
  bool trackNewestCoarse(FrameHessianT* newFrameHessian, SE3T& lastToNew_out, AffLightT& aff_g2l_out, int coarsestLvl, Vec5T minResForAbort,
                         void* /*wrap*/ = nullptr) {
    if (!slot_of) throw Error("trackNewestCoarse: slot_of not set");
    return trackNewestCoarse(slot_of(newFrameHessian), newFrameHessian->ab_exposure, lastToNew_out, aff_g2l_out, coarsestLvl, minResForAbort);
  }
  // bool trackNewestCoarse(...) with the frame given by its pyramid slot
  template <class Vec5T>
  bool trackNewestCoarse(int newFrame_slot, float newFrame_ab_exposure, SE3T& lastToNew_out, AffLightT& aff_g2l_out, int coarsestLvl,
                         const Vec5T& minResForAbort) {
    prm_.new_exposure = newFrame_ab_exposure;
    prm_.coarsestLvl = coarsestLvl;
    for (int i = 0; i < 5; i++) prm_.minResForAbort[i] = minResForAbort[i];
    sdso_se3_t T = toAbi(lastToNew_out);
    sdso_aff_t aff{aff_g2l_out.a, aff_g2l_out.b};
    sdso_track_result_t out;
    if (forkLive) dev_.check(sdso_g2o_track_newest_coarse(dev_.ctx(), ref_slot_, newFrame_slot, &prm_, &T, &aff, &out), "sdso_g2o_track_newest_coarse");
    else dev_.check(sdso_track_newest_coarse(dev_.ctx(), ref_slot_, newFrame_slot, &prm_, &T, &aff, &out), "sdso_track_newest_coarse");
    for (int i = 0; i < 5; i++) lastResiduals[i] = out.lastResiduals[i];
    for (int i = 0; i < 3; i++) lastFlowIndicators[i] = out.lastFlowIndicators[i];
    lastToNew_out = fromAbi<SE3T, Mat33T, Vec3T>(T);
    aff_g2l_out.a = aff.a; aff_g2l_out.b = aff.b;
    lastStats = out;
    return out.good != 0;
  }
  // FullSystem::trackNewCoarse STEP2-4 (FullSystem.cpp:436-511) as one member: the loop over lastF_2_fh_tries — trackNewestCoarse per try
  // under the running achievedRes, the winner, the carry, the stop at lastCoarseRMSE[0] * setting_reTrackThreshold, the ending without a
  // good try — on the device (sdso_track_new_coarse: try 0 alone; the other tries, where the loop goes on, in one launch).  TriesT is the
  // reference's std::vector<SE3, Eigen::aligned_allocator<SE3>>; Vec5T / Vec3FlowT its Vec5 / Vec3.
  //   in    fh, lastF_2_fh_tries, aff_last_2_l, coarsestLvl (pyrLevelsUsed-1, :448), reTrackThreshold (setting_reTrackThreshold)
  //   inout lastCoarseRMSE (:499, :511)
  //   out   lastF_2_fh, aff_g2l, flowVecs, achievedRes, tryIterations; returns haveOneGood (the caller prints the BIG ERROR of :504)
  // Afterwards lastResiduals / lastFlowIndicators are those of the last try the loop ran, as in the reference, and firstCoarseRMSE is
  // set as :528-529 set it.  lastTries holds one record per try (ran, what the loop saw, the abort level).  With forkLive the tries run
  // the fork's live body (sdso_g2o_track_new_coarse: one EdgeSE3PosePhotoDSO per point, g2o's Levenberg-Marquardt), under the same rules.
  template <class FrameHessianT, class TriesT, class Vec5T, class Vec3FlowT>
  bool trackNewCoarse(FrameHessianT* fh, const TriesT& lastF_2_fh_tries, const AffLightT& aff_last_2_l, int coarsestLvl, Vec5T& lastCoarseRMSE,
                      float reTrackThreshold, SE3T& lastF_2_fh, AffLightT& aff_g2l, Vec3FlowT& flowVecs, Vec5T& achievedRes, int& tryIterations) {
    if (!slot_of) throw Error("trackNewCoarse: slot_of not set");
    return trackNewCoarse(slot_of(fh), fh->ab_exposure, lastF_2_fh_tries, aff_last_2_l, coarsestLvl, lastCoarseRMSE, reTrackThreshold, lastF_2_fh, aff_g2l,
                          flowVecs, achievedRes, tryIterations);
  }
  // ... with the frame given by its pyramid slot
  template <class TriesT, class Vec5T, class Vec3FlowT>
  bool trackNewCoarse(int newFrame_slot, float newFrame_ab_exposure, const TriesT& lastF_2_fh_tries, const AffLightT& aff_last_2_l, int coarsestLvl,
                      Vec5T& lastCoarseRMSE, float reTrackThreshold, SE3T& lastF_2_fh, AffLightT& aff_g2l, Vec3FlowT& flowVecs, Vec5T& achievedRes,
                      int& tryIterations) {
    prm_.new_exposure = newFrame_ab_exposure;
    prm_.coarsestLvl = coarsestLvl;
    std::vector<sdso_se3_t> tries;
    for (const auto& T : lastF_2_fh_tries) tries.push_back(toAbi(T));
    const sdso_aff_t aff0{aff_last_2_l.a, aff_last_2_l.b};
    double rmse[5];
    for (int i = 0; i < 5; i++) rmse[i] = lastCoarseRMSE[i];
    lastTries.assign(tries.size(), sdso_track_try_t{});
    if (forkLive)
      dev_.check(sdso_g2o_track_new_coarse(dev_.ctx(), ref_slot_, newFrame_slot, &prm_, (int)tries.size(), tries.data(), &aff0, rmse, (double)reTrackThreshold,
                                           &lastTriesResult, lastTries.data()), "sdso_g2o_track_new_coarse");
    else
      dev_.check(sdso_track_new_coarse(dev_.ctx(), ref_slot_, newFrame_slot, &prm_, (int)tries.size(), tries.data(), &aff0, rmse, (double)reTrackThreshold,
                                       &lastTriesResult, lastTries.data()), "sdso_track_new_coarse");
    const sdso_track_tries_result_t& r = lastTriesResult;
    const sdso_track_try_t& last = lastTries[r.tryIterations - 1];       // the tracker's members after the loop: the last try it ran
    for (int i = 0; i < 5; i++) { lastResiduals[i] = last.lastResiduals[i]; achievedRes[i] = r.achievedRes[i]; lastCoarseRMSE[i] = rmse[i]; }   // :511
    for (int i = 0; i < 3; i++) { lastFlowIndicators[i] = last.lastFlowIndicators[i]; flowVecs[i] = r.flowVecs[i]; }
    lastF_2_fh = fromAbi<SE3T, Mat33T, Vec3T>(r.pose);
    aff_g2l.a = r.aff.a; aff_g2l.b = r.aff.b;
    tryIterations = r.tryIterations;
    if (firstCoarseRMSE < 0) firstCoarseRMSE = r.achievedRes[0];         // :528-529
    return r.haveOneGood != 0;
  }
  std::vector<sdso_track_try_t> lastTries;
  sdso_track_tries_result_t lastTriesResult{};
  // calcRes + calcGSSSE for one (level, pose): what the LM loop evaluates; returns calcRes' Vec6
  void calcResAndGS(int lvl, int newFrame_slot, float newFrame_ab_exposure, const SE3T& refToNew, const AffLightT& aff_g2l, float levelCutoffRepeat,
                    double H_out[64], double b_out[8], double res6[6], int* buf_warped_n = nullptr) {
    prm_.new_exposure = newFrame_ab_exposure;
    sdso_track_eval_t ev;
    const sdso_se3_t T = toAbi(refToNew);
    const sdso_aff_t a{aff_g2l.a, aff_g2l.b};
    sdso_track_make_eval(&prm_, lvl, &T, &a, levelCutoffRepeat, &ev);
    dev_.check(sdso_track_calc_res_gs(dev_.ctx(), ref_slot_, newFrame_slot, &ev, H_out, b_out, res6, buf_warped_n, nullptr), "sdso_track_calc_res_gs");
  }

  // false: DSO-native LM (the body kept as comments at CoarseTracker.cpp:908-1024).  true: the fork's live body — one
  // EdgeSE3PosePhotoDSO per point and g2o's Levenberg-Marquardt, 2 iterations per level (CoarseTracker.cpp:834-1047).
  bool forkLive = false;
  // public outputs of the reference (CoarseTracker.h:98-113)
  double lastResiduals[5];
  double lastFlowIndicators[3];
  double firstCoarseRMSE = -1;
  int refFrameID = -1;
  sdso_track_result_t lastStats{};
  sdso_track_params_t& params() { return prm_; }
  AffLightT lastRef_aff_g2l{};

 private:
  template <class FrameHessianT>
  void installRef_(FrameHessianT* lastRef, int n, const int* u, const int* v, const float* new_idepth, const float* weight) {
    dev_.check(sdso_track_make_ref(dev_.ctx(), ref_slot_, slot_of(lastRef), n, u, v, new_idepth, weight, pc_n), "sdso_track_make_ref");
    newRef_(lastRef);
  }
  // The bookkeeping after a new template (:821-825); lastRef is null where the caller gave a slot only.  Only the frame form keeps lastRef_aff_g2l.
  void newRef_(const void* lastRef, int lastRef_slot, int refFrameID_, float ab_exposure, const AffLightT& aff_g2l) {
    lastRef_ = lastRef; lastRef_slot_ = lastRef_slot; idepth0_ok_ = false; adopted_ = false;
    refFrameID = refFrameID_;
    prm_.ref_exposure = ab_exposure;
    prm_.ref_aff_g2l.a = aff_g2l.a; prm_.ref_aff_g2l.b = aff_g2l.b;
    firstCoarseRMSE = -1;
  }
  template <class FrameHessianT> void newRef_(FrameHessianT* lastRef) {
    lastRef_aff_g2l = lastRef->aff_g2l();
    newRef_(lastRef, slot_of(lastRef), lastRef->shell->id, lastRef->ab_exposure, lastRef_aff_g2l);
  }
  void requireMap_(const char* who) const {
    if (!publish_) throw Error(std::string(who) + ": the tracker was constructed without publishDepthImages");
    if (lastRef_slot_ < 0 || adopted_) throw Error(std::string(who) + ": no template built on the device is installed");
  }
  Device& dev_;
  int ref_slot_;
  bool publish_;
  const void* lastRef_ = nullptr;
  int lastRef_slot_ = -1;
  bool adopted_ = false;                                     // the template came through adoptRef: lastRef_slot_ is the builder's, the map too
  std::vector<float> idepth0_;                               // idepth[0] on the host, as debugPlotIDepthMapFloat wraps it
  bool idepth0_ok_ = false;
  sdso_track_params_t prm_;
};
}  // namespace sdso_shim
