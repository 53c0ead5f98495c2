// sdso_shim.h — header-only C++ host layer that keeps the reference's call surface
// (CoarseTracker / EnergyFunctional / ImmaturePoint) on top of the C-ABI of
// libsdso_hip.so.  It is written against the reference's member NAMES through templates, so the same
// header compiles
//   * inside the reference tree against its real types (Eigen/Sophus: SE3 = Sophus::SE3d, AffLight,
//     FrameHessian, CalibHessian, EnergyFunctional, EFFrame/EFPoint/EFResidual, ImmaturePoint), and
//   * in this repository against the small stand-ins of host/test_shim.cpp (Eigen is not available here).
// Nothing here computes on the CPU what the library computes on the GPU; the shim only marshals.
//
// Reference signatures mirrored (paths under /root/reference/src):
//   bool CoarseTracker::trackNewestCoarse(FrameHessian*, SE3&, AffLight&, int coarsestLvl, Vec5 minResForAbort, ...)   FullSystem/CoarseTracker.h:62-66
//   void CoarseTracker::makeK(CalibHessian*)                                                                        FullSystem/CoarseTracker.h:76
//   Vec6 CoarseTracker::calcRes(int lvl, SE3 refToNew, AffLight aff_g2l, float cutoffTH) + calcGSSSE(lvl,H,b,...)    FullSystem/CoarseTracker.cpp:600, :537
//   void EnergyFunctional::solveSystemF(int iteration, double lambda, CalibHessian*)                                 OptimizationBackend/EnergyFunctional.h:74
//   void EnergyFunctional::marginalizePointsF()                                                                      OptimizationBackend/EnergyFunctional.h:69
//   float FullSystem::optimize(int mnumOptIts)                                                                       FullSystem/FullSystemOptimize.cpp:871
//   ImmaturePointStatus ImmaturePoint::traceStereo(FrameHessian* frame, Mat33f K, bool mode_right)                   FullSystem/ImmaturePoint.h:89
//   void CoarseTracker::setCoarseTrackingRef(std::vector<FrameHessian*>, FrameHessian* fh_right, CalibHessian)        FullSystem/CoarseTracker.h:71-72
//   void CoarseTracker::setCTRefForFirstFrame(std::vector<FrameHessian*>)                                           FullSystem/CoarseTracker.cpp:794-805
//   void CoarseTracker::debugPlotIDepthMap(float* minID, float* maxID, std::vector<IOWrap::Output3DWrapper*>& wraps)    FullSystem/CoarseTracker.h:94, CoarseTracker.cpp:1071-1176
//   void CoarseTracker::debugPlotIDepthMapFloat(std::vector<IOWrap::Output3DWrapper*>& wraps)                         FullSystem/CoarseTracker.h:95, CoarseTracker.cpp:1178-1188
//   double PointFrameResidual::linearize(CalibHessian*) / void applyRes(bool)                                        FullSystem/Residuals.h:103, :113
//   AccumulatedTopHessianSSE::{setZero, addPoint<mode>, addPointsInternal<mode>, stitchDouble, stitchDoubleMT}        OptimizationBackend/AccumulatedTopHessian.h:66-97, :162-169
//   AccumulatedSCHessianSSE::{setZero, addPoint, addPointsInternal, stitchDouble, stitchDoubleMT}                     OptimizationBackend/AccumulatedSCHessian.h:66-96, :155-160
//   EnergyFunctional::{calcLEnergyF_MT, calcMEnergyF, setDeltaF, setAdjointsF}                                       OptimizationBackend/EnergyFunctional.h:75-86
//   CoarseDistanceMap::{makeK, makeDistanceMap, addIntoDistFinal, fwdWarpedIDDistFinal, K, Ki}                          FullSystem/CoarseTracker.h:165-197
//   void FullSystem::activatePointsMT() STEP 1-2                                                                      FullSystem/FullSystem.cpp:796-902
//   the tail of optimizeImmaturePoint + STEP 4 of activatePointsMT into the resident window (WindowedBA::updateActivated)   FullSystem/FullSystemOptPoint.cpp:196-237, FullSystem.cpp:919-945
//   void FullSystem::makeNewTraces(FrameHessian*, FrameHessian*, float*), traceNewCoarseNonKey / traceNewCoarseKey(fh, fh_right)    FullSystem/FullSystem.cpp:1600, :632, :745
//   the loop of void FullSystem::stereoMatch(ImageAndExposure*, ImageAndExposure*, int, cv::Mat&)                      FullSystem/FullSystem.cpp:579-613
//   Undistort::{undistort<T>, getK, getSize, getOriginalSize, getBl, isValid, loadPhotometricCalibration}               util/Undistort.h:63-104
//   void KeyFrameDisplay::setFromKF(FrameHessian* fh, CalibHessian* HCalib)                                          IOWrapper/Pangolin/KeyFrameDisplay.h:62, .cpp:85-165
//   bool KeyFrameDisplay::refreshPC(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity)  IOWrapper/Pangolin/KeyFrameDisplay.h:66, .cpp:174-323
//   void CoarseInitializer::setFirstStereo(CalibHessian*, FrameHessian* newFrameHessian, FrameHessian* newFrameHessian_Right)   FullSystem/CoarseInitializer.h:108, .cpp:838-1034
//   STEP 3 of void FullSystem::initializeFromInitializer(FrameHessian* newFrame)                                  FullSystem/FullSystem.cpp:1533-1573
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/sdso_abi.h"

namespace sdso_shim {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

// One GPU + stream.  The reference serialises tracking under trackMutex and mapping under mapMutex;
// use one Device per such domain (or one shared Device and the same mutexes).
class Device {
 public:
  explicit Device(int ordinal = 0) {
    if (sdso_ctx_create(ordinal, &ctx_) != SDSO_OK) throw Error("sdso_ctx_create failed: no usable HIP device (there is no CPU fallback)");
  }
  ~Device() { sdso_ctx_destroy(ctx_); }
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;
  sdso_ctx* ctx() const { return ctx_; }
  void check(int rc, const char* what) const {
    if (rc != SDSO_OK) throw Error(std::string(what) + ": " + sdso_last_error(ctx_));
  }
  // FrameHessian::dIp mirrors: immutable after makeImages, so upload once per frame (key = shell->id / frameID)
  template <class FrameHessianT>
  void uploadFrame(int slot, const FrameHessianT* fh, int levels, const int* w, const int* h) {
    std::vector<const float*> p(levels);
    for (int l = 0; l < levels; l++) p[l] = reinterpret_cast<const float*>(fh->dIp[l]);  // Eigen::Vector3f is 3 packed floats
    check(sdso_upload_pyramid(ctx_, slot, levels, w, h, p.data()), "sdso_upload_pyramid");
  }
  void releaseFrame(int slot) { sdso_release_pyramid(ctx_, slot); }
  // traceStereo's sub-pixel refinement: false = DSO-native GN (ImmaturePoint.cpp:707-769), true = the fork's g2o GN on
  // EdgeTracePointUVDSO (ImmaturePoint.cpp:309-412)
  // Multi-GPU: one process per GPU; rank 0 makes the id (static uniqueId()), the caller ships the 128 bytes to the other ranks,
  // then every rank calls commInit (collective).  RCCL is resolved at run time; a missing librccl is an error, not a fallback.
  static void uniqueId(unsigned char id[128]) {
    if (sdso_comm_unique_id(id) != SDSO_OK) throw Error("sdso_comm_unique_id failed (librccl.so.1 not loadable?)");
  }
  void commInit(int nranks, int rank, const unsigned char id[128]) { check(sdso_comm_init(ctx_, nranks, rank, id), "sdso_comm_init"); }
  void setForkLiveTraceRefinement(bool on) { check(sdso_trace_set_gn_mode(ctx_, on ? 1 : 0), "sdso_trace_set_gn_mode"); }

 private:
  sdso_ctx* ctx_ = nullptr;
};

// ---- SE3 / AffLight marshalling (Sophus::SE3d API: rotationMatrix()(i,j), translation()[i], ctor(R, t))
template <class SE3T>
inline sdso_se3_t toAbi(const SE3T& T) {
  sdso_se3_t o;
  const auto R = T.rotationMatrix();
  const auto t = T.translation();
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o.R[i * 3 + j] = R(i, j); o.t[i] = t[i]; }
  return o;
}
template <class SE3T, class Mat33T, class Vec3T>
inline SE3T fromAbi(const sdso_se3_t& a) {
  Mat33T R;
  Vec3T t;
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = a.R[i * 3 + j]; t[i] = a.t[i]; }
  return SE3T(R, t);
}

// =================================================================================== CoarseTracker
// Drop-in for the tracking half of dso::CoarseTracker.  Template parameters are the reference's own
// types; Mat33/Vec3 are the Eigen double types used to rebuild an SE3.
template <class SE3T, class AffLightT, class Mat33T, class Vec3T>
class CoarseTracker {
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
  template <class CalibHessianT>
  void makeK(CalibHessianT* HCalib, int pyrLevelsUsed, int w0, int h0) {
    prm_.levels = pyrLevelsUsed;
    prm_.w[0] = w0; prm_.h[0] = h0;
    prm_.fx[0] = HCalib->fxl(); prm_.fy[0] = HCalib->fyl(); prm_.cx[0] = HCalib->cxl(); prm_.cy[0] = HCalib->cyl();
    for (int l = 1; l < pyrLevelsUsed; ++l) {
      prm_.w[l] = w0 >> l; prm_.h[l] = h0 >> l;
      prm_.fx[l] = prm_.fx[l - 1] * 0.5; prm_.fy[l] = prm_.fy[l - 1] * 0.5;
      prm_.cx[l] = (prm_.cx[0] + 0.5) / ((int)1 << l) - 0.5;
      prm_.cy[l] = (prm_.cy[0] + 0.5) / ((int)1 << l) - 0.5;
    }
  }
  // The template point cloud the reference builds in makeCoarseDepthL0 (CoarseTracker.cpp:507-532):
  // pc_u/pc_v/pc_idepth/pc_color[lvl], pc_n[lvl].  Called once per new reference keyframe.
  void setCoarseTrackingRef(int lvl, int pc_n, const float* pc_u, const float* pc_v, const float* pc_idepth, const float* pc_color,
                            float lastRef_ab_exposure, const AffLightT& lastRef_aff_g2l_, int refFrameID_) {
    dev_.check(sdso_track_set_ref(dev_.ctx(), ref_slot_, lvl, pc_n, pc_u, pc_v, pc_idepth, pc_color), "sdso_track_set_ref");
    newRef_(nullptr, -1);                                           // a template from the host carries no level-0 map
    prm_.ref_exposure = lastRef_ab_exposure;
    prm_.ref_aff_g2l.a = lastRef_aff_g2l_.a; prm_.ref_aff_g2l.b = lastRef_aff_g2l_.b;
    refFrameID = refFrameID_;
    firstCoarseRMSE = -1;
  }
  // makeCoarseDepthL0 (CoarseTracker.cpp:275-534) from STEP1's per-point results: integer pixel (u,v) on lastRef, the
  // (stereo-refined) new_idepth and weight = sqrtf(1e-3 / (HdiF + 1e-12)).  Splat, pyramid, dilation, normalisation and
  // the raster-order compaction run on the device; pc_n[lvl] comes back for the reference's bookkeeping.
  void makeCoarseDepthL0(int lastRef_slot, int n, const int* u, const int* v, const float* new_idepth, const float* weight, int* pc_n,
                         float lastRef_ab_exposure, const AffLightT& lastRef_aff_g2l_, int refFrameID_) {
    dev_.check(sdso_track_make_ref(dev_.ctx(), ref_slot_, lastRef_slot, n, u, v, new_idepth, weight, pc_n), "sdso_track_make_ref");
    newRef_(nullptr, lastRef_slot);
    prm_.ref_exposure = lastRef_ab_exposure;
    prm_.ref_aff_g2l.a = lastRef_aff_g2l_.a; prm_.ref_aff_g2l.b = lastRef_aff_g2l_.b;
    refFrameID = refFrameID_;
    firstCoarseRMSE = -1;
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
      const float K4[4] = {Hcalib.fxl(), Hcalib.fyl(), Hcalib.cxl(), Hcalib.cyl()};
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
    newRef_(lastRef, slot_of(lastRef));
    refFrameID = lastRef->shell->id;                         // :821-825
    lastRef_aff_g2l = lastRef->aff_g2l();
    prm_.ref_exposure = lastRef->ab_exposure;
    prm_.ref_aff_g2l.a = lastRef_aff_g2l.a; prm_.ref_aff_g2l.b = lastRef_aff_g2l.b;
    firstCoarseRMSE = -1;
  }
  // void setCTRefForFirstFrame(std::vector<FrameHessian*> frameHessians) — CoarseTracker.cpp:794-805 with makeCoarseDepthForFirstFrame
  // (:138-271): the first keyframe's own points at int(u + 0.5f), their idepth, no stereo refinement; STEP2-5 are makeCoarseDepthL0's.
  template <class FrameHessianT>
  void setCTRefForFirstFrame(std::vector<FrameHessianT*> frameHessians) {
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
  // void debugPlotIDepthMap(float* minID_pt, float* maxID_pt, std::vector<IOWrap::Output3DWrapper*>& wraps) — CoarseTracker.cpp:1071-1176,
  // what FullSystem::makeKeyFrame calls on coarseTracker_forNewKF for every keyframe (FullSystem.cpp:1444).  The sort of :1078-1088, the
  // smoothing of :1094-1117 and the image of :1119-1163 run on the device on the map the latest template kept (sdso_track_depth_image);
  // here: the early return of :1072, the MinimalImageB3 the wrappers receive, and the pushes of :1167-1168.  The call also brings the
  // float map to the host, where debugPlotIDepthMapFloat finds it.  MinimalImageB3T is named by the caller: dso::MinimalImageB3.
  // (debugSaveImages' writeImage, :1170-1174, is the caller's: the image is the one the wrappers were handed.)
  template <class MinimalImageB3T, class WrapT>
  void debugPlotIDepthMap(float* minID_pt, float* maxID_pt, std::vector<WrapT*>& wraps) {
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
  template <class MinimalImageFT, class FrameHessianT, class WrapT>
  void debugPlotIDepthMapFloat(std::vector<WrapT*>& wraps) {
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
    newRef_(lastRef, slot_of(lastRef));
    refFrameID = lastRef->shell->id;                         // :821-825
    lastRef_aff_g2l = lastRef->aff_g2l();
    prm_.ref_exposure = lastRef->ab_exposure;
    prm_.ref_aff_g2l.a = lastRef_aff_g2l.a; prm_.ref_aff_g2l.b = lastRef_aff_g2l.b;
    firstCoarseRMSE = -1;
  }
  // a new template: lastRef (null where the caller gave a slot only) and its pyramid slot, for the two debugPlot members
  void newRef_(const void* lastRef, int lastRef_slot) { lastRef_ = lastRef; lastRef_slot_ = lastRef_slot; idepth0_ok_ = false; }
  void requireMap_(const char* who) const {
    if (!publish_) throw Error(std::string(who) + ": the tracker was constructed without publishDepthImages");
    if (lastRef_slot_ < 0) throw Error(std::string(who) + ": no template built on the device is installed");
  }
  Device& dev_;
  int ref_slot_;
  bool publish_;
  const void* lastRef_ = nullptr;
  int lastRef_slot_ = -1;
  std::vector<float> idepth0_;                               // idepth[0] on the host, as debugPlotIDepthMapFloat wraps it
  bool idepth0_ok_ = false;
  sdso_track_params_t prm_;
};

// =================================================================================== EnergyFunctional
// Flattens the reference's pointer graph (EnergyFunctional::frames -> EFFrame::points -> EFPoint::residualsAll,
// i.e. makeIDX order, EnergyFunctional.cpp:998-1018) into sdso_ba_window_t and drives the device window.
// slot_of(FrameHessian*) returns the pyramid slot the frame was uploaded to.
template <class EnergyFunctionalT, class CalibHessianT>
class WindowedBA {
 public:
  WindowedBA(Device& dev, int win_id) : dev_(dev), win_(win_id) {}

  template <class SlotOf>
  void upload(EnergyFunctionalT* ef, CalibHessianT* HCalib, int w, int h, int solverMode, double affineOptModeA, double affineOptModeB,
              bool forceAcceptStep, SlotOf slot_of) {
    const int nf = (int)ef->frames.size();
    FrameCols& F = up_frames_; PointCols& P = up_points_; ResCols& R = up_res_;
    F.clear(); P.clear(); R.clear(); points_.clear(); residuals_.clear();
    for (int f = 0; f < nf; f++) F.push(ef->frames[f]->data, slot_of);
    for (int f = 0; f < nf; f++)
      for (auto* p : ef->frames[f]->points) {
        const int pi = (int)P.u.size();
        P.push(p->data, f);
        points_.push_back(p);
        for (auto* r : p->residualsAll) {                  // residualsAll order: the order of the reference's per-point float sums
          R.push(pi, r->target->idx, r->data);
          residuals_.push_back(r);
        }
      }
    sdso_ba_window_t W; std::memset(&W, 0, sizeof(W));
    W.nf = nf; W.np = (int)P.u.size(); W.nr = (int)R.point.size(); W.w = w; W.h = h;
    for (int i = 0; i < 4; i++) { W.calib_value_scaled[i] = HCalib->value_scaled[i]; W.calib_value_zero[i] = HCalib->value_zero[i]; }
    W.evalPT = F.evalPT.data(); W.state = F.state.data(); W.state_zero = F.state_zero.data();
    W.ab_exposure = F.exposure.data(); W.frameEnergyTH = F.energyTH.data(); W.frameID = F.frameID.data(); W.frame_slot = F.slots.data();
    W.u = P.u.data(); W.v = P.v.data(); W.idepth = P.idepth.data(); W.idepth_zero = P.idepth_zero.data();
    W.color = P.color.data(); W.weights = P.weights.data(); W.host = P.host.data(); W.hasDepthPrior = P.prior.data();
    W.res_point = R.point.data(); W.res_target = R.target.data(); W.res_state = R.state.data();
    W.maxRelBaseline = P.maxRelBaseline.data(); W.numGoodResiduals = P.numGood.data(); W.res_isNew = R.isNew.data();
    const int n = 8 * nf + 4;
    HM_.assign((size_t)n * n, 0); bM_.assign(n, 0);
    for (int i = 0; i < n; i++) { bM_[i] = ef->bM[i]; for (int j = 0; j < n; j++) HM_[(size_t)i * n + j] = ef->HM(i, j); }
    W.HM = HM_.data(); W.bM = bM_.data();
    W.solverMode = solverMode; W.affineOptModeA = affineOptModeA; W.affineOptModeB = affineOptModeB; W.forceAcceptStep = forceAcceptStep ? 1 : 0;
    dev_.check(sdso_ba_upload_window(dev_.ctx(), win_, &W), "sdso_ba_upload_window");
    nf_ = nf; resInM_seen_ = 0; ef_ = ef;
    reindex_();
    lin_valid_ = app_valid_ = acc_valid_ = marg_valid_ = false;
    frames_.assign(ef->frames.begin(), ef->frames.end());
    clearPending_();
    window_serial_++;
  }

  // Vec3 FullSystem::linearizeAll(false): returns lastEnergyP
  double linearizeAll() {
    double e = 0;
    dev_.check(sdso_ba_linearize(dev_.ctx(), win_, &e), "sdso_ba_linearize");
    lin_valid_ = app_valid_ = acc_valid_ = marg_valid_ = false;
    return e;
  }
  // applyRes_Reductor(true, ...)
  void applyRes() { dev_.check(sdso_ba_apply_res(dev_.ctx(), win_), "sdso_ba_apply_res"); app_valid_ = acc_valid_ = marg_valid_ = false; }

  // double PointFrameResidual::linearize(CalibHessian* HCalib) (Residuals.h:103, Residuals.cpp:83-336) and void applyRes(bool copyJacobians)
  // (Residuals.h:113, Residuals.cpp:367-385) PER OBJECT, the way linearizeAll_Reductor / applyRes_Reductor call them
  // (FullSystemOptimize.cpp:52-96): the device linearises / applies the whole window at the first call after a change and every call
  // hands its own residual's results out — state_NewEnergy, state_NewEnergyWithOutlier, state_NewState; then state_state, state_energy,
  // EFResidual::isActiveAndIsGoodNEW.  A linearised residual (EFResidual::isLinearized) is not touched — the reference's loops run over
  // activeResiduals, which holds none (FullSystemOptimize.cpp:880-889) —: both members return before any write.
  template <class PointFrameResidualT>
  double linearize(PointFrameResidualT* r, CalibHessianT* /*HCalib*/) {
    if (r->efResidual->isLinearized) return 0.0;
    requireNoPendingEdit_("linearize");
    if (!lin_valid_) {
      const int nr = (int)residuals_.size();
      linearizeAll();
      l_state_.assign(nr, 0); l_energy_.assign(nr, 0.f); l_energyWO_.assign(nr, 0.f);
      dev_.check(sdso_ba_get_linearization(dev_.ctx(), win_, nullptr, l_state_.data(), l_energy_.data(), l_energyWO_.data(), nullptr, nullptr), "sdso_ba_get_linearization");
      lin_valid_ = true;
    }
    const int i = index_of_(r);
    using ResStateT = std::decay_t<decltype(r->state_NewState)>;
    r->state_NewState = static_cast<ResStateT>(l_state_[i]);
    r->state_NewEnergyWithOutlier = l_energyWO_[i];
    // (an OOB residual returns its old state_energy without touching state_NewEnergy: Residuals.cpp:88-91, :226)
    if (l_state_[i] == 1) return r->state_energy;
    r->state_NewEnergy = l_energy_[i];
    return r->state_NewEnergy;
  }
  template <class PointFrameResidualT>
  void applyRes(PointFrameResidualT* r, bool copyJacobians) {
    if (r->efResidual->isLinearized) return;
    if (!copyJacobians) {   // Residuals.cpp:382-384 alone: setState(state_NewState); state_energy = state_NewEnergy — no OOB test, isActiveAndIsGoodNEW untouched
      r->state_state = r->state_NewState;
      r->state_energy = r->state_NewEnergy;
      return;
    }
    if (!app_valid_) {
      requireNoPendingEdit_("applyRes");
      const int nr = (int)residuals_.size();
      applyRes();
      a_state_.assign(nr, 0); a_act_.assign(nr, 0);
      dev_.check(sdso_ba_get_residual_state(dev_.ctx(), win_, a_state_.data(), a_act_.data(), nullptr), "sdso_ba_get_residual_state");
      app_valid_ = true;
    }
    const int i = index_of_(r);
    using ResStateT = std::decay_t<decltype(r->state_state)>;
    if ((int)r->state_state == 1) return;                     // `if(state_state == ResState::OOB) return;` — can never go back from OOB
    r->state_state = static_cast<ResStateT>(a_state_[i]);
    r->state_energy = r->state_NewEnergy;
    r->efResidual->isActiveAndIsGoodNEW = a_act_[i] != 0;
  }
  // EnergyFunctional::solveSystemF(iteration, lambda, HCalib): fills lastX; frame / calib / point steps are fetched below
  // Multi-GPU: when this process holds only a contiguous range of allPoints, sum the packed accumulators over the
  // ranks before the stitch — what stitchDoubleMT does with the per-thread copies (AccumulatedTopHessian.cpp:299-308), across GPUs.
  // Device::commInit must have been called (sdso_comm_unique_id / sdso_comm_init); a no-op without a communicator.
  void allreduce() {
    int nranks = 0;
    dev_.check(sdso_comm_info(dev_.ctx(), &nranks, nullptr), "sdso_comm_info");
    if (nranks > 1) dev_.check(sdso_ba_allreduce_window(dev_.ctx(), win_), "sdso_ba_allreduce_window");
  }
  void solveSystemF(int iteration, double lambda, std::vector<double>& lastX, std::vector<double>& frame_step, double calib_step[4]) {
    const int n = 8 * nf_ + 4;
    lastX.assign(n, 0); frame_step.assign(nf_ * 8, 0);
    ensureAccumulated();
    dev_.check(sdso_ba_solve(dev_.ctx(), win_, iteration, lambda, lastX.data(), nullptr, nullptr, frame_step.data(), calib_step), "sdso_ba_solve");
  }
  // void EnergyFunctional::solveSystemF(int iteration, double lambda, CalibHessian* HCalib) — EnergyFunctional.h:74, EnergyFunctional.cpp:838-995
  // with resubstituteF_MT (:272-341) — verbatim: everything the reference's function leaves in its objects is written into them:
  //   ef->lastX, lastHS, lastbS (:909-910, :992); ef->resInA / resInL (:219, :241); HCalib->step = -x.head<CPARS>() (:279);
  //   every EFFrame::data->step.head<8>() = -x.segment<8>(CPARS + 8 idx), tail<2>() = 0 (:283-286);
  //   every PointHessian::step (:336-338), EFPoint::HdiF / bdSumF (AccumulatedSCHessian.cpp:58-65)
  void solveSystemF(int iteration, double lambda, CalibHessianT* HCalib) {
    const int n = 8 * nf_ + 4, np = (int)points_.size();
    std::vector<double> x(n), HS((size_t)n * n), bS(n), fstep(nf_ * 8);
    double cstep[4];
    ensureAccumulated();
    dev_.check(sdso_ba_solve(dev_.ctx(), win_, iteration, lambda, x.data(), HS.data(), bS.data(), fstep.data(), cstep), "sdso_ba_solve");
    ef_->lastX.resize(n); ef_->lastbS.resize(n); ef_->lastHS.resize(n, n);
    fill_(ef_->lastX, x.data(), n); fill_(ef_->lastbS, bS.data(), n); fill_(ef_->lastHS, HS.data(), n, n);
    for (int i = 0; i < 4; i++) HCalib->step[i] = cstep[i];
    for (int f = 0; f < nf_; f++) {
      auto* fh = ef_->frames[f]->data;
      for (int i = 0; i < 8; i++) fh->step[i] = fstep[f * 8 + i];
      fh->step[8] = 0; fh->step[9] = 0;
    }
    std::vector<float> pstep(np), hdi(np), bds(np);
    if (np) {
      dev_.check(sdso_ba_get_point_steps(dev_.ctx(), win_, pstep.data()), "sdso_ba_get_point_steps");
      dev_.check(sdso_ba_get_point_terms(dev_.ctx(), win_, hdi.data(), bds.data(), nullptr, nullptr, nullptr), "sdso_ba_get_point_terms");
    }
    for (int p = 0; p < np; p++) { points_[p]->data->step = pstep[p]; points_[p]->HdiF = hdi[p]; points_[p]->bdSumF = bds[p]; }
    int ra = 0, rl = 0;
    dev_.check(sdso_ba_get_counts(dev_.ctx(), win_, &ra, &rl, nullptr), "sdso_ba_get_counts");
    ef_->resInA = ra; ef_->resInL = rl;
  }
  // double EnergyFunctional::calcLEnergyF_MT() / double calcMEnergyF() — EnergyFunctional.h:82-83, EnergyFunctional.cpp:420-442, :344-351
  double calcLEnergyF_MT() { double el = 0; dev_.check(sdso_ba_calc_energies(dev_.ctx(), win_, &el, nullptr), "sdso_ba_calc_energies"); return el; }
  double calcMEnergyF() { double em = 0; dev_.check(sdso_ba_calc_energies(dev_.ctx(), win_, nullptr, &em), "sdso_ba_calc_energies"); return em; }
  // void EnergyFunctional::setAdjointsF(CalibHessian* Hcalib) — EnergyFunctional.h:86, EnergyFunctional.cpp:41-119: the window's adjoints
  // (computed at upload / whenever the device loop moved the states) into ef->adHost / adTarget / adHostF / adTargetF, [h + t * nFrames]
  void setAdjointsF(CalibHessianT* /*Hcalib*/) {
    const int nf = nf_;
    std::vector<double> aH((size_t)nf * nf * 64), aT((size_t)nf * nf * 64);
    dev_.check(sdso_ba_get_tables(dev_.ctx(), win_, nullptr, aH.data(), aT.data(), nullptr), "sdso_ba_get_tables");
    using M88 = std::remove_pointer_t<decltype(ef_->adHost)>;
    using M88f = std::remove_pointer_t<decltype(ef_->adHostF)>;
    if (ef_->adHost != 0) delete[] ef_->adHost;
    if (ef_->adTarget != 0) delete[] ef_->adTarget;
    if (ef_->adHostF != 0) delete[] ef_->adHostF;
    if (ef_->adTargetF != 0) delete[] ef_->adTargetF;
    ef_->adHost = new M88[nf * nf]; ef_->adTarget = new M88[nf * nf]; ef_->adHostF = new M88f[nf * nf]; ef_->adTargetF = new M88f[nf * nf];
    for (int k = 0; k < nf * nf; k++)
      for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) {
          ef_->adHost[k](i, j) = aH[(size_t)k * 64 + i * 8 + j]; ef_->adTarget[k](i, j) = aT[(size_t)k * 64 + i * 8 + j];
          ef_->adHostF[k](i, j) = (float)aH[(size_t)k * 64 + i * 8 + j]; ef_->adTargetF[k](i, j) = (float)aT[(size_t)k * 64 + i * 8 + j];
        }
  }
  // void EnergyFunctional::setDeltaF(CalibHessian* HCalib) — EnergyFunctional.h:75, EnergyFunctional.cpp:173-207: adHTdeltaF[h + t * nFrames],
  // cDeltaF, EFFrame::delta / delta_prior, EFPoint::deltaF
  void setDeltaF(CalibHessianT* /*HCalib*/) {
    const int nf = nf_, np = (int)points_.size();
    std::vector<float> adhtd((size_t)nf * nf * 8), pd(np);
    std::vector<double> fd(nf * 8), fdp(nf * 8);
    float cd[4];
    dev_.check(sdso_ba_get_tables(dev_.ctx(), win_, nullptr, nullptr, nullptr, adhtd.data()), "sdso_ba_get_tables");
    dev_.check(sdso_ba_get_deltas(dev_.ctx(), win_, cd, fd.data(), fdp.data(), pd.data()), "sdso_ba_get_deltas");
    using M18f = std::remove_pointer_t<decltype(ef_->adHTdeltaF)>;
    if (ef_->adHTdeltaF != 0) delete[] ef_->adHTdeltaF;
    ef_->adHTdeltaF = new M18f[nf * nf];
    for (int k = 0; k < nf * nf; k++) for (int j = 0; j < 8; j++) ef_->adHTdeltaF[k](0, j) = adhtd[(size_t)k * 8 + j];
    for (int i = 0; i < 4; i++) ef_->cDeltaF[i] = cd[i];
    for (int f = 0; f < nf; f++) for (int i = 0; i < 8; i++) { ef_->frames[f]->delta[i] = fd[f * 8 + i]; ef_->frames[f]->delta_prior[i] = fdp[f * 8 + i]; }
    for (int p = 0; p < np; p++) points_[p]->deltaF = pd[p];
  }
  // the device pass behind accumulateAF_MT + accumulateLF_MT + accumulateSCF_MT: runs once per linearised / applied state
  void ensureAccumulated() {
    if (acc_valid_) return;
    dev_.check(sdso_ba_accumulate(dev_.ctx(), win_), "sdso_ba_accumulate");
    allreduce();
    acc_valid_ = true; marg_valid_ = false;
  }
  // marginalizePointsF's device pass for the points the accumulator façades collected (addPoint<2>): see AccumulatedTopHessianSSE below
  // (type-erased form for the accumulator façade, which holds the points as `const void*`)
  void ensureMarginalizedErased(const std::vector<const void*>& flagged) {
    if (marg_valid_) return;
    std::vector<uint8_t> flag(points_.size(), 0);
    for (const void* p : flagged) flag[point_index_.at(p)] = 1;
    const int before = countOf(2);
    dev_.check(sdso_ba_marginalize_points(dev_.ctx(), win_, flag.data(), HM_.data(), bM_.data()), "sdso_ba_marginalize_points");
    last_marg_res_ = countOf(2) - before;
    marg_valid_ = true; acc_valid_ = lin_valid_ = app_valid_ = false;
  }
  void requireMarginalized() const { if (!marg_valid_) throw Error("AccumulatedSCHessianSSE: the marginalisation pass has not run (stitch the top accumulator first, EnergyFunctional.cpp:707-708)"); }
  int lastMargResiduals() const { return last_marg_res_; }
  const std::vector<double>& HM() const { return HM_; }
  const std::vector<double>& bM() const { return bM_; }
  template <class MatXX, class VecX> void stitchedSystem(int which, MatXX& H, VecX& b) { stitched_(which, H, b); }
  int countOf(int which) {                                    // 0 resInA, 1 resInL, 2 residuals marginalised through this window so far
    int c[3] = {0, 0, 0};
    dev_.check(sdso_ba_get_counts(dev_.ctx(), win_, &c[0], &c[1], &c[2]), "sdso_ba_get_counts");
    return c[which];
  }
  int nFrames() const { return nf_; }
  // void EnergyFunctional::accumulateAF_MT(MatXX& H, VecX& b, bool MT) / accumulateLF_MT / accumulateSCF_MT (EnergyFunctional.cpp:212-269,
  // EnergyFunctional.h:103-105): what the reference's callers get back is the STITCHED system of AccumulatedTopHessianSSE::stitchDoubleMT
  // (mode 0 without priors, mode 1 with priors) / AccumulatedSCHessianSSE::stitchDoubleMT.  The device accumulates all three in one pass
  // (sdso_ba_accumulate) and its solver never materialises them; these members run the stitch kernels on demand.  MatXX / VecX: anything
  // with resize(rows[, cols]) and operator()(i[, j]) — Eigen's, or the stand-ins of host/test_shim.cpp.  `MT` is ignored.
  void accumulateAll() { acc_valid_ = false; ensureAccumulated(); }
  template <class MatXX, class VecX> void accumulateAF_MT(MatXX& H, VecX& b, bool /*MT*/) { stitched_(0, H, b); }
  template <class MatXX, class VecX> void accumulateLF_MT(MatXX& H, VecX& b, bool /*MT*/) { stitched_(1, H, b); }
  template <class MatXX, class VecX> void accumulateSCF_MT(MatXX& H, VecX& b, bool /*MT*/) { stitched_(2, H, b); }
  // float FullSystem::optimize(int mnumOptIts) — FullSystemOptimize.cpp:871-1041 from `activeResiduals.clear()` (:880) through the closing
  // `linearizeAll(true)` (:1008) — on the uploaded window, with EVERYTHING that function leaves behind written back into the reference's
  // own objects (sdso_ba_get_post_state):
  //   CalibHessian      setValue (value, value_scaled, ...), step                                   :218-222 via doStepFromBackup
  //   FrameHessian      setState (state, state_scaled, PRE_worldToCam, PRE_camToWorld), step; the newest frame's setEvalPT (:997-1003);
  //                     its frameEnergyTH (setNewFrameEnergyTH of the closing linearizeAll)
  //   PointHessian      setIdepth + setIdepthZero (:268-272), step, idepth_hessian, maxRelBaseline, numGoodResiduals (:64-77,
  //                     AccumulatedSCHessian.cpp:44-58); EFPoint::HdiF, bdSumF
  //   PointFrameResidual state_state / state_NewState, state_energy, centerProjectedTo, projectedTo; EFResidual::isActiveAndIsGoodNEW
  //   PointHessian::lastResiduals[k].second (:165-172); for every residual on toRemove: lastResiduals[k].first = 0,
  //                     ef->dropResidual(r->efResidual), deleteOut(ph->residuals, k) (:176-195) — in activeResiduals order
  //   EnergyFunctional  lastX, lastHS, lastbS, resInA, resInL
  // Left to the caller exactly as in the reference: `ef->setAdjointsF(&Hcalib); setPrecalcValues();` (:1005-1007, host tables other host
  // code reads), the isLost test, statistics_lastFineTrackRMSE and the shell poses (:1010-1037).  Not written back: the
  // RawResidualJacobian records (EFResidual::J) — only the accumulators this library replaces read them.
  // Returns sqrtf(lastEnergy[0] / (patternNum * ef->resInA)) like the reference (:1039); lastResult carries lastEnergy[0].
  float optimize(int mnumOptIts, EnergyFunctionalT* ef, CalibHessianT* HCalib) {
    requireNoPendingEdit_("optimize");
    const int nf = nf_, np = (int)points_.size(), nr = (int)residuals_.size(), n = 8 * nf + 4;
    sdso_ba_opt_result_t out;
    lin_valid_ = app_valid_ = acc_valid_ = marg_valid_ = false;
    if (nf < 2) { lastResult = sdso_ba_opt_result_t{0, 0, 0, 0}; lastRemoved = 0; return 0.f; }   // `if(frameHessians.size() < 2) return 0;` (:873-874): nothing is touched
    dev_.check(sdso_ba_optimize(dev_.ctx(), win_, mnumOptIts, nullptr, nullptr, nullptr, &out), "sdso_ba_optimize");
    std::vector<float> idp(np), pstep(np), hdi(np), bds(np), idh(np), mrb(np), energy(nr), cpt((size_t)nr * 3), prj((size_t)nr * 16), eth(nf);
    std::vector<int> ngood(np);
    std::vector<uint8_t> rs(nr), act(nr), rem(nr);
    std::vector<double> st(nf * 10), stz(nf * 10), ev(nf * 12), fstep(nf * 10), lx(n), lhs((size_t)n * n), lbs(n);
    sdso_ba_post_state_t P;
    std::memset(&P, 0, sizeof(P));
    P.idepth = idp.data(); P.step = pstep.data(); P.HdiF = hdi.data(); P.bdSumF = bds.data(); P.idepth_hessian = idh.data();
    P.maxRelBaseline = mrb.data(); P.numGoodResiduals = ngood.data();
    P.state_state = rs.data(); P.isActiveAndIsGoodNEW = act.data(); P.state_energy = energy.data(); P.toRemove = rem.data();
    if (writeBackProjections) { P.centerProjectedTo = cpt.data(); P.projectedTo = prj.data(); }
    P.state = st.data(); P.state_zero = stz.data(); P.evalPT = ev.data(); P.frame_step = fstep.data(); P.frameEnergyTH = eth.data();
    P.lastX = lx.data(); P.lastHS = lhs.data(); P.lastbS = lbs.data();
    dev_.check(sdso_ba_get_post_state(dev_.ctx(), win_, &P), "sdso_ba_get_post_state");
    // ---- calibration and frames
    {
      auto v = HCalib->value_zero;                         // a VecC to fill
      for (int i = 0; i < 4; i++) v[i] = P.calib_value[i];
      HCalib->setValue(v);
      for (int i = 0; i < 4; i++) HCalib->step[i] = P.calib_step[i];
    }
    for (int f = 0; f < nf; f++) {
      auto* fh = ef->frames[f]->data;
      auto s = fh->get_state();                            // a Vec10 to fill
      for (int i = 0; i < 10; i++) s[i] = st[f * 10 + i];
      if (f == nf - 1) {
        // setEvalPT(PRE_worldToCam at the loop's final state, {0,..,0, a, b, 0, 0}) (:997-1003)
        sdso_se3_t T;
        std::memcpy(T.R, &ev[f * 12], 72); std::memcpy(T.t, &ev[f * 12 + 9], 24);
        fh->setEvalPT(like(fh->get_worldToCam_evalPT(), T), s);
      } else fh->setState(s);
      for (int i = 0; i < 10; i++) fh->step[i] = fstep[f * 10 + i];
      fh->frameEnergyTH = eth[f];
    }
    // ---- points
    for (int p = 0; p < np; p++) {
      auto* efp = points_[p];
      auto* ph = efp->data;
      ph->setIdepth(idp[p]); ph->setIdepthZero(idp[p]);
      ph->step = pstep[p];
      if (writeBackPointStats) { ph->idepth_hessian = idh[p]; ph->maxRelBaseline = mrb[p]; ph->numGoodResiduals = ngood[p]; }
      efp->HdiF = hdi[p]; efp->bdSumF = bds[p];
    }
    // ---- residuals
    for (int i = 0; i < nr; i++) {
      auto* r = residuals_[i];
      auto* pfr = r->data;
      if (r->isLinearized) continue;                       // not in activeResiduals (:880-889): optimize() never touches it
      using ResStateT = std::decay_t<decltype(pfr->state_state)>;
      pfr->state_state = static_cast<ResStateT>(rs[i]);
      pfr->state_NewState = static_cast<ResStateT>(rs[i]);
      pfr->state_energy = energy[i]; pfr->state_NewEnergy = energy[i];
      r->isActiveAndIsGoodNEW = act[i] != 0;
      if (act[i] && writeBackProjections) {
        for (int k = 0; k < 3; k++) pfr->centerProjectedTo[k] = cpt[(size_t)i * 3 + k];
        for (int k = 0; k < 8; k++) { pfr->projectedTo[k][0] = prj[(size_t)i * 16 + 2 * k]; pfr->projectedTo[k][1] = prj[(size_t)i * 16 + 2 * k + 1]; }
      }
      auto* ph = pfr->point;                               // :165-172
      if (ph->lastResiduals[0].first == pfr) ph->lastResiduals[0].second = pfr->state_state;
      else if (ph->lastResiduals[1].first == pfr) ph->lastResiduals[1].second = pfr->state_state;
    }
    int nResRemoved = 0;
    for (int i = 0; i < nr; i++) {                         // :176-195
      if (!rem[i] || residuals_[i]->isLinearized) continue;
      auto* pfr = residuals_[i]->data;
      auto* ph = pfr->point;
      if (ph->lastResiduals[0].first == pfr) ph->lastResiduals[0].first = 0;
      else if (ph->lastResiduals[1].first == pfr) ph->lastResiduals[1].first = 0;
      for (unsigned int k = 0; k < ph->residuals.size(); k++)
        if (ph->residuals[k] == pfr) {
          ef->dropResidual(pfr->efResidual);
          res_index_.erase(pfr); residuals_[i] = nullptr; pending_drop_res_.push_back(i);   // stage 1 of the next update(), in toRemove order
          delete ph->residuals[k];                         // deleteOut<PointFrameResidual>(ph->residuals, k), FullSystem.h:62-71
          ph->residuals[k] = ph->residuals.back();
          ph->residuals.pop_back();
          nResRemoved++;
          break;
        }
    }
    // (dropResidual deleted some residuals: their slots in residuals_ are null until update() — or upload() — brings the device window in line)
    lastRemoved = nResRemoved;
    // ---- EnergyFunctional
    ef->lastX.resize(n); ef->lastbS.resize(n); ef->lastHS.resize(n, n);
    fill_(ef->lastX, lx.data(), n); fill_(ef->lastbS, lbs.data(), n); fill_(ef->lastHS, lhs.data(), n, n);
    ef->resInA = P.resInA; ef->resInL = P.resInL;
    lastResult = out;
    return (float)out.rmse;
  }
  int lastRemoved = 0;
  // false: optimize() does not fetch PointFrameResidual::centerProjectedTo / projectedTo (nr x 19 floats evaluated and downloaded by
  // sdso_ba_get_post_state) and leaves them as they were.  Their only reader on the keyframe path is makeCoarseDepthL0, so switch it off
  // exactly when the tracking reference comes from CoarseTracker::setCoarseTrackingRef(ba, ...) and no other code of the caller reads them.
  bool writeBackProjections = true;
  // false: optimize() leaves PointHessian::idepth_hessian / maxRelBaseline / numGoodResiduals as they were (their one reader on the keyframe
  // path is flagPointsForRemoval, which the two members below decide on the device; the window carries all three from keyframe to keyframe
  // through update()).  idepth, step, HdiF and bdSumF are written back either way: other host code reads them.  The download is the same
  // (sdso_ba_get_post_state copies the per-point arrays together); what goes is the host loop's three stores per point.  Needs update(),
  // not upload(), for the next keyframe: an upload would read the stale members.
  bool writeBackPointStats = true;
  // ---- FullSystem::removeOutliers (FullSystemOptimize.cpp:1063-1084) and FullSystem::flagPointsForRemoval (FullSystem.cpp:965-1056) with the
  // reference's effects on the pointer graph, decided on the device (sdso_ba_flag_points): nothing per point is read from the PointHessians
  // but lastResiduals.  frameHessians: std::vector<FrameHessian*>-like, in window order; of a frame the members flaggedForMarginalization,
  // pointHessians, pointHessiansOut, pointHessiansMarginalized are touched.
  //   removeOutliers(frameHessians)        after optimize(), before anything edits the device window: makes the one device call and keeps the
  //                                        decisions; points without a residual get PS_DROP, go to pointHessiansOut and leave pointHessians by
  //                                        swap-with-back (:1073-1079).  Its ef->dropPointsF() (:1083) waits for the one that follows
  //                                        flagPointsForRemoval: the dropped points have left pointHessians, nothing in between meets them,
  //                                        and one window edit holds one dropPointsF sweep (two sweeps order EFFrame::points differently)
  //   flagPointsForRemoval(frameHessians)  consumes the kept decisions: stateFlag, pointHessiansOut / pointHessiansMarginalized, the
  //                                        null-then-compact of :1042-1053, the four counters.  The caller goes on with willDropPoints +
  //                                        ef->dropPointsF(), update() and marginalizePointsF (which holds :1012-1021)
  // frame_marg = flaggedForMarginalization; last_gone[2p+k] = lastResiduals[k].second where .first == 0 (a residual that has left: optimize()
  // cleared it, or an earlier keyframe did), 255 where it is live — then the window holds that residual and knows its state.
  int setting_minGoodActiveResForMarg = 3, setting_minGoodResForMarg = 4;   // settings.cpp:82-83
  float setting_minIdepthH_marg = 50;                                       // settings.cpp:57
  int numPointsDropped = 0;                                                 // removeOutliers' (:1064)
  int flag_oob = 0, flag_in = 0, flag_inin = 0, flag_nores = 0;             // flagPointsForRemoval's (FullSystem.cpp:981)
  template <class FrameHessians>
  void removeOutliers(FrameHessians& frameHessians) {
    flags_pending_ = false;
    const int nf = nf_, np = (int)points_.size();
    if ((int)frameHessians.size() != nf) throw Error("removeOutliers: frameHessians is not the device window's frame list");
    if (!pending_rm_points_.empty() || !pending_drop_flags_.empty() || !pending_rm_frames_.empty())
      throw Error("removeOutliers: points or frames left the EnergyFunctional since optimize(): call it right after optimize()");
    std::vector<uint8_t> frame_marg(nf), last_gone((size_t)np * 2, 255);
    for (int f = 0; f < nf; f++) frame_marg[f] = frameHessians[f]->flaggedForMarginalization ? 1 : 0;
    for (int p = 0; p < np; p++) {
      auto* ph = points_[p]->data;
      for (int k = 0; k < 2; k++) {
        auto* first = ph->lastResiduals[k].first;
        if (!first) { last_gone[(size_t)p * 2 + k] = (uint8_t)ph->lastResiduals[k].second; continue; }
        auto it = res_index_.find(first);
        if (it == res_index_.end() || nf - 1 - k < 0 || residuals_[it->second]->target != frames_[nf - 1 - k])
          throw Error("removeOutliers: a live lastResiduals[k].first does not observe frame nf-1-k of the device window");
      }
    }
    sdso_ba_flag_points_t F;
    F.frame_marg = frame_marg.data(); F.last_gone = last_gone.data();
    F.minGoodActiveResForMarg = setting_minGoodActiveResForMarg; F.minGoodResForMarg = setting_minGoodResForMarg; F.minIdepthH_marg = setting_minIdepthH_marg;
    flag_decisions_.assign((size_t)np, 0);
    dev_.check(sdso_ba_flag_points(dev_.ctx(), win_, &F, flag_decisions_.data(), nullptr, nullptr), "sdso_ba_flag_points");
    flags_pending_ = true; flags_serial_ = window_serial_;
    numPointsDropped = 0;
    for (auto* fh : frameHessians)
      for (unsigned int i = 0; i < fh->pointHessians.size(); i++) {
        auto* ph = fh->pointHessians[i];
        if (ph == 0) continue;
        if (decisionOf_(ph->efPoint, "removeOutliers") == SDSO_PT_DROP_NO_RESIDUAL) {      // ph->residuals.size() == 0 (:1073)
          fh->pointHessiansOut.push_back(ph);
          setStateFlag_(ph->efPoint, 2);
          fh->pointHessians[i] = fh->pointHessians.back();
          fh->pointHessians.pop_back();
          i--;
          numPointsDropped++;
        }
      }
  }
  template <class FrameHessians>
  void flagPointsForRemoval(FrameHessians& frameHessians) {
    if (!flags_pending_) throw Error("flagPointsForRemoval: no decisions are pending: removeOutliers() makes them, once per optimize()");
    if (flags_serial_ != window_serial_) throw Error("flagPointsForRemoval: the device window was edited since removeOutliers() (update() / upload() come after it)");
    flag_oob = flag_in = flag_inin = flag_nores = 0;
    for (auto* host : frameHessians) {
      for (unsigned int i = 0; i < host->pointHessians.size(); i++) {
        auto* ph = host->pointHessians[i];
        if (ph == 0) continue;
        const int d = decisionOf_(ph->efPoint, "flagPointsForRemoval");
        if (d == SDSO_PT_DROP_NEGATIVE || d == SDSO_PT_DROP_NO_RESIDUAL) {                 // FullSystem.cpp:997-1002
          host->pointHessiansOut.push_back(ph);
          setStateFlag_(ph->efPoint, 2);
          host->pointHessians[i] = 0;
          flag_nores++;
        } else if (d != SDSO_PT_KEEP) {                                                    // :1004-1041
          flag_oob++;
          if (d == SDSO_PT_MARGINALIZE || d == SDSO_PT_DROP_WEAK) {
            flag_in++;
            if (d == SDSO_PT_MARGINALIZE) {
              flag_inin++;
              setStateFlag_(ph->efPoint, 1);
              host->pointHessiansMarginalized.push_back(ph);
            } else {
              setStateFlag_(ph->efPoint, 2);
              host->pointHessiansOut.push_back(ph);
            }
          } else {
            host->pointHessiansOut.push_back(ph);
            setStateFlag_(ph->efPoint, 2);
          }
          host->pointHessians[i] = 0;
        }
      }
      for (int i = 0; i < (int)host->pointHessians.size(); i++)                            // :1044-1051
        if (host->pointHessians[i] == 0) {
          host->pointHessians[i] = host->pointHessians.back();
          host->pointHessians.pop_back();
          i--;
        }
    }
    flags_pending_ = false;
  }
  int win() const { return win_; }
  // index of an EFPoint in the device window's point order, -1 when it is not part of it
  int pointIndexOf(const void* efPoint) const { auto it = point_index_.find(efPoint); return it == point_index_.end() ? -1 : it->second; }
  // EnergyFunctional::marginalizePointsF() (EnergyFunctional.cpp:663-736): points with stateFlag == PS_MARGINALIZE; updates ef->HM / ef->bM /
  // ef->resInM.  The re-linearisation + fixLinearizationF that FullSystem::flagPointsForRemoval runs on those points beforehand
  // (FullSystem.cpp:1012-1021) is part of the call.  Call upload() first: optimize() dropped residuals and the reference drops points in between
  // (removeOutliers, flagPointsForRemoval + dropPointsF), so the window of the optimize call no longer matches the EnergyFunctional.
  // The caller goes on with the reference's removePoint loop (:730-735).
  template <class IsMarg>
  void marginalizePointsF(EnergyFunctionalT* ef, IsMarg is_marg) {
    requireNoPendingEdit_("marginalizePointsF");
    std::vector<uint8_t> flag(points_.size());
    for (size_t p = 0; p < points_.size(); p++) flag[p] = is_marg(points_[p]) ? 1 : 0;
    const int n = 8 * nf_ + 4;
    dev_.check(sdso_ba_marginalize_points(dev_.ctx(), win_, flag.data(), HM_.data(), bM_.data()), "sdso_ba_marginalize_points");
    marg_valid_ = true; acc_valid_ = lin_valid_ = app_valid_ = false;
    fill_(ef->bM, bM_.data(), n); fill_(ef->HM, HM_.data(), n, n);
    int resInM = 0;                                        // resInM += accSSE_top_A->nres[0] (EnergyFunctional.cpp:704)
    dev_.check(sdso_ba_get_counts(dev_.ctx(), win_, nullptr, nullptr, &resInM), "sdso_ba_get_counts");
    ef->resInM += resInM - resInM_seen_; resInM_seen_ = resInM;
  }
  sdso_ba_opt_result_t lastResult{};

  // ---- the window stays on the device from one call to the next (sdso_ba_window_update) instead of being flattened and uploaded again.
  // The reference deletes the objects it removes, so the shim is told about a removal BEFORE the reference performs it (an index is
  // looked up while the pointer is still valid, and a later object at the same address cannot be mistaken for it):
  //   optimize()                      notes the toRemove drops itself (stage 1)
  //   willRemovePoint(p)              before each ef->removePoint(p) of marginalizePointsF's loop (EnergyFunctional.cpp:692-696): stage 2
  //   willDropPoints(is_drop)         before ef->dropPointsF() (:739-752), is_drop(p) = p->stateFlag == EFPointStatus::PS_DROP: stage 3
  //   marginalizeFrame(ef, f)         in place of the algebra of EnergyFunctional::marginalizeFrame (:560-628) on the device-resident prior
  //                                   (sdso_ba_marginalize_frame_dev), ef->HM / ef->bM written back; the caller goes on with :631-660.
  //                                   The residuals into that frame are dropped by FullSystem::marginalizeFrame as before: stage 4
  //   update(ef, slot_of)             after the reference inserted what the next keyframe brings (insertFrame, insertResidual, insertPoint):
  //                                   frames / residuals / points the shim has not seen are stages 5-7, in makeIDX order
  // update() leaves points_ / residuals_ and their index maps describing the edited window (checked against sdso_ba_window_get_order).
  template <class EFPointT>
  void willRemovePoint(EFPointT* p) {
    const int i = point_index_.at(p);
    pending_rm_points_.push_back(i);
    forgetPoint_(i);
  }
  template <class IsDrop>
  void willDropPoints(IsDrop is_drop) {
    if (pending_drop_flags_.empty()) pending_drop_flags_.assign(points_.size(), 0);
    for (size_t i = 0; i < points_.size(); i++)
      if (points_[i] && is_drop(points_[i])) { pending_drop_flags_[i] = 1; forgetPoint_((int)i); }
  }
  template <class EFFrameT>
  void marginalizeFrame(EnergyFunctionalT* ef, EFFrameT* f) {
    int old_idx = -1, idx = 0;                             // idx counts the frames the prior still covers (sdso_abi.h)
    for (size_t k = 0; k < frames_.size(); k++) {
      if (frames_[k] == f) { old_idx = (int)k; break; }
      if (std::find(pending_rm_frames_.begin(), pending_rm_frames_.end(), (int)k) == pending_rm_frames_.end()) idx++;
    }
    if (old_idx < 0) throw Error("marginalizeFrame: the frame is not part of the uploaded window");
    const int left = nf_ - (int)pending_rm_frames_.size() - 1, m = 8 * left + 4;
    std::vector<double> H((size_t)m * m), b(m);
    dev_.check(sdso_ba_marginalize_frame_dev(dev_.ctx(), win_, idx, H.data(), b.data()), "sdso_ba_marginalize_frame_dev");
    ef->HM.resize(m, m); ef->bM.resize(m);
    fill_(ef->bM, b.data(), m); fill_(ef->HM, H.data(), m, m);
    pending_rm_frames_.push_back(old_idx);
    for (size_t i = 0; i < residuals_.size(); i++)         // FullSystem::marginalizeFrame drops them next (FullSystemMarginalize.cpp:150-180)
      if (residuals_[i] && residuals_[i]->target == f) { res_index_.erase(residuals_[i]->data); residuals_[i] = nullptr; }
  }
  //   updateActivated(ef, slot_of, frameHessians, n_records)
  //                                   update() for the keyframe whose new points come from ImmaturePoints::activatePointsMT on this Device:
  //                                   stage 7 is taken from the activation's records where they lie (sdso_ba_window_update_activated), so
  //                                   no float of an activated point is read from the caller's objects.  The caller has run its loop over
  //                                   the Activated records with their integer members alone — status 1: a PointHessian on a.host, a
  //                                   PointFrameResidual per IN entry of a.res_state, ef->insertPoint / insertResidual (FullSystemOptPoint.cpp:
  //                                   196-237, FullSystem.cpp:923-933) — frameHessians is the vector that activation walked and n_records the
  //                                   size of the vector it returned.  Returns
  //                                   act_index: the k-th appended point is entry act_index[k] of the Activated vector; the order check
  //                                   below holds the caller's objects against what the device appended.
  template <class SlotOf>
  void update(EnergyFunctionalT* ef, SlotOf slot_of) { update_(ef, slot_of, nullptr, 0); }
  template <class SlotOf, class FrameHessianT>
  std::vector<int> updateActivated(EnergyFunctionalT* ef, SlotOf slot_of, const std::vector<FrameHessianT*>& frameHessians, size_t n_records) {
    std::vector<const void*> act(frameHessians.begin(), frameHessians.end());
    return update_(ef, slot_of, &act, n_records);
  }
  // the index of ef frame `f` in the device window (after upload() / update()); -1: not part of it
  template <class EFFrameT>
  int frameIndex(const EFFrameT* f) const {
    for (size_t k = 0; k < frames_.size(); k++) if (frames_[k] == f) return (int)k;
    return -1;
  }
  int windowId() const { return win_; }
  int frameCount() const { return nf_; }

 private:
  template <class SlotOf>
  std::vector<int> update_(EnergyFunctionalT* ef, SlotOf slot_of, const std::vector<const void*>* act_frames, size_t act_records) {
    const int nf_old = nf_;
    std::unordered_map<const void*, int> frame_old;        // EFFrame* -> index before the call (appended frames: nf_old + k)
    for (int k = 0; k < nf_old; k++)
      if (std::find(pending_rm_frames_.begin(), pending_rm_frames_.end(), k) == pending_rm_frames_.end()) frame_old[frames_[k]] = k;
    // ---- stage 5: frames the shim has not seen (insertFrame appends, EnergyFunctional.cpp:465-466)
    FrameCols F; int n_add_frames = 0;
    for (auto* f : ef->frames) {
      if (frame_old.count(f)) { if (n_add_frames) throw Error("update: a known frame follows a new one"); continue; }
      F.push(f->data, slot_of);
      frame_old[f] = nf_old + n_add_frames++;
    }
    auto frame_of = [&](const void* f) {
      auto it = frame_old.find(f);
      if (it == frame_old.end()) throw Error("update: a residual or point names a frame that is not part of the window (a frame that left?)");
      return it->second;
    };
    // ---- stages 6 and 7: the residuals and points the shim has not seen, in makeIDX order (EnergyFunctional.cpp:998-1018)
    ResCols ar, pr; PointCols pt;                          // stage 6: residuals into known points; stage 7: the new points and theirs
    std::vector<int> want_point, want_res;                 // what sdso_ba_window_get_order must say
    decltype(points_) new_points; decltype(residuals_) new_residuals;
    for (auto* f : ef->frames)
      for (auto* p : f->points) {
        auto it = point_index_.find(p);
        new_points.push_back(p);
        if (it != point_index_.end()) {
          want_point.push_back(it->second);
          for (auto* r : p->residualsAll) {
            new_residuals.push_back(r);
            auto ir = res_index_.find(r->data);
            if (ir != res_index_.end()) { want_res.push_back(ir->second); continue; }
            want_res.push_back(-1 - (int)ar.point.size());
            ar.push(it->second, frame_of(r->target), r->data);
          }
        } else {
          const int q = (int)pt.host.size();
          want_point.push_back(-1 - q);
          pt.push(p->data, frame_of(f));
          for (auto* r : p->residualsAll) {
            new_residuals.push_back(r);
            want_res.push_back(-(int)pr.point.size() - 1);   // (+ the stage-6 count, added below)
            pr.push(q, frame_of(r->target), r->data);
          }
        }
      }
    {  // stage-7 residual ids follow stage 6's
      size_t i = 0;
      for (size_t p = 0; p < new_points.size(); p++) {
        const size_t cnt = new_points[p]->residualsAll.size();
        if (want_point[p] < 0) for (size_t k = 0; k < cnt; k++) want_res[i + k] -= (int)ar.point.size();
        i += cnt;
      }
    }
    sdso_ba_window_edit_t E;
    std::memset(&E, 0, sizeof(E));
    E.n_drop_res = (int)pending_drop_res_.size(); E.drop_res = pending_drop_res_.data();
    E.n_remove_points = (int)pending_rm_points_.size(); E.remove_points = pending_rm_points_.data();
    E.drop_point = pending_drop_flags_.empty() ? nullptr : pending_drop_flags_.data();
    E.n_remove_frames = (int)pending_rm_frames_.size(); E.remove_frames = pending_rm_frames_.data();
    E.n_add_frames = n_add_frames;
    E.evalPT = F.evalPT.data(); E.state = F.state.data(); E.state_zero = F.state_zero.data();
    E.ab_exposure = F.exposure.data(); E.frameEnergyTH = F.energyTH.data(); E.frameID = F.frameID.data(); E.frame_slot = F.slots.data();
    E.n_add_res = (int)ar.point.size(); E.add_res_point = ar.point.data(); E.add_res_target = ar.target.data();
    E.add_res_state = ar.state.data(); E.add_res_isNew = ar.isNew.data();
    E.n_add_points = (int)pt.host.size(); E.pt_host = pt.host.data();
    E.pt_u = pt.u.data(); E.pt_v = pt.v.data(); E.pt_idepth = pt.idepth.data(); E.pt_idepth_zero = pt.idepth_zero.data();
    E.pt_color = pt.color.data(); E.pt_weights = pt.weights.data();
    E.pt_hasDepthPrior = pt.prior.data(); E.pt_maxRelBaseline = pt.maxRelBaseline.data(); E.pt_numGoodResiduals = pt.numGood.data();
    E.n_pt_res = (int)pr.point.size(); E.pt_res_point = pr.point.data(); E.pt_res_target = pr.target.data();
    E.pt_res_state = pr.state.data(); E.pt_res_isNew = pr.isNew.data();
    std::vector<int> act_index;
    if (!act_frames) {
      dev_.check(sdso_ba_window_update(dev_.ctx(), win_, &E), "sdso_ba_window_update");
    } else {
      // act_frame: the window frame (numbering before the call) of every frame the activation walked
      std::vector<int> act_frame;
      for (const void* fh : *act_frames) {
        int at = -1;
        for (auto* f : ef->frames) if ((const void*)f->data == fh) at = frame_of(f);
        if (at < 0) throw Error("updateActivated: a frame of the activation is not part of the EnergyFunctional");
        // (the reference's frameHessians and ef->frames are in one order; the order check below relies on it: the device numbers the
        // appended points in toOptimize order, which is then the order the walk above met the caller's objects in)
        if (!act_frame.empty() && at <= act_frame.back()) throw Error("updateActivated: the activation's frames are not in the EnergyFunctional's order");
        act_frame.push_back(at);
      }
      const int want_np = E.n_add_points, want_nr = E.n_pt_res;
      E.n_add_points = 0; E.n_pt_res = 0;                    // stage 7 comes from the records
      int n_pt = 0, n_res = 0;
      std::vector<int> idx_all(std::max<size_t>(act_records, 1), -1);   // the library writes one entry per appended point, at most one per record
      dev_.check(sdso_ba_window_update_activated(dev_.ctx(), win_, &E, act_frame.data(), &n_pt, &n_res, idx_all.data()), "sdso_ba_window_update_activated");
      if (n_pt != want_np || n_res != want_nr) throw Error("updateActivated: the caller inserted other points / residuals than the activation made");
      act_index.assign(idx_all.begin(), idx_all.begin() + n_pt);
    }
    // ---- the device's order is the EnergyFunctional's, or the two have drifted apart
    const int nf2 = (int)ef->frames.size();
    std::vector<int> fs(nf2), ps(new_points.size()), rs(new_residuals.size());
    dev_.check(sdso_ba_window_get_order(dev_.ctx(), win_, fs.data(), ps.data(), rs.data()), "sdso_ba_window_get_order");
    for (int k = 0; k < nf2; k++) {
      const int o = frame_old.at(ef->frames[k]);
      if (fs[k] != (o < nf_old ? o : -1 - (o - nf_old))) throw Error("update: the device window's frames differ from the EnergyFunctional's");
    }
    if (ps != want_point || rs != want_res) throw Error("update: the device window's order differs from the EnergyFunctional's (a removal the shim was not told about?)");
    points_.swap(new_points); residuals_.swap(new_residuals);
    reindex_();
    frames_.assign(ef->frames.begin(), ef->frames.end());
    nf_ = nf2; ef_ = ef;
    HM_.assign((size_t)(8 * nf2 + 4) * (8 * nf2 + 4), 0.0); bM_.assign(8 * nf2 + 4, 0.0);   // (host copies of the prior: sized per window, filled by marginalizePointsF)
    clearPending_();
    window_serial_++;
    lin_valid_ = app_valid_ = acc_valid_ = marg_valid_ = false;
    return act_index;
  }

  // optimize() / willRemovePoint / willDropPoints / marginalizeFrame left null slots in points_ / residuals_: the members that walk those
  // lists need update() (or upload()) first
  void requireNoPendingEdit_(const char* who) const {
    if (!pending_drop_res_.empty() || !pending_rm_points_.empty() || !pending_drop_flags_.empty() || !pending_rm_frames_.empty())
      throw Error(std::string(who) + ": the EnergyFunctional changed since the device window was brought in line: call update() (or upload()) first");
  }
  void clearPending_() { pending_drop_res_.clear(); pending_rm_points_.clear(); pending_drop_flags_.clear(); pending_rm_frames_.clear(); }
  void forgetPoint_(int i) {                               // the point and its residuals leave the index maps before the reference deletes them
    for (auto* r : points_[i]->residualsAll) {
      auto it = res_index_.find(r->data);
      if (it != res_index_.end()) { residuals_[it->second] = nullptr; res_index_.erase(it); }
    }
    point_index_.erase(points_[i]); points_[i] = nullptr;
  }
  // the kept decision of a point that is still part of the device window's numbering
  int decisionOf_(const void* efPoint, const char* who) const {
    auto it = point_index_.find(efPoint);
    if (!efPoint || it == point_index_.end()) throw Error(std::string(who) + ": a point of pointHessians is not part of the device window");
    return flag_decisions_[(size_t)it->second];
  }
  // EFPointStatus (EnergyFunctionalStructs.h:97): PS_GOOD = 0, PS_MARGINALIZE = 1, PS_DROP = 2
  template <class EFPointT> static void setStateFlag_(EFPointT* p, int v) { p->stateFlag = static_cast<std::decay_t<decltype(p->stateFlag)>>(v); }
  std::vector<uint8_t> flag_decisions_;                    // sdso_ba_flag_points of the latest removeOutliers(), device point order
  bool flags_pending_ = false;
  int window_serial_ = 0, flags_serial_ = 0;               // upload() / update() count; the count the decisions were made at
  std::vector<int> pending_drop_res_, pending_rm_points_, pending_rm_frames_;
  std::vector<uint8_t> pending_drop_flags_;
  std::vector<const void*> frames_;                        // EFFrame* of the uploaded window, in order
  template <class MatXX, class VecX> void stitched_(int which, MatXX& H, VecX& b) {
    const int n = 8 * nf_ + 4;
    std::vector<double> Hs((size_t)n * n), bs(n);
    double* Hp[3] = {nullptr, nullptr, nullptr};
    double* bp[3] = {nullptr, nullptr, nullptr};
    Hp[which] = Hs.data(); bp[which] = bs.data();
    dev_.check(sdso_ba_get_stitched(dev_.ctx(), win_, Hp[0], bp[0], Hp[1], bp[1], Hp[2], bp[2]), "sdso_ba_get_stitched");
    H.resize(n, n); b.resize(n);
    fill_(b, bs.data(), n); fill_(H, Hs.data(), n, n);
  }
  template <class PointFrameResidualT> int index_of_(PointFrameResidualT* r) const {
    auto it = res_index_.find(r);
    if (it == res_index_.end()) throw Error("residual is not part of the uploaded window");
    return it->second;
  }
  Device& dev_;
  int win_, nf_ = 0, resInM_seen_ = 0;
  EnergyFunctionalT* ef_ = nullptr;
  int last_marg_res_ = 0;
  bool lin_valid_ = false, app_valid_ = false, acc_valid_ = false, marg_valid_ = false;
  std::unordered_map<const void*, int> res_index_, point_index_;
  std::vector<uint8_t> l_state_, a_state_, a_act_;
  std::vector<float> l_energy_, l_energyWO_;
  // ---- a frame's, a point's and a residual's record as columns of the ABI's arrays: upload() fills one set for the window, update() one for its gains
  struct FrameCols {
    std::vector<double> evalPT, state, state_zero; std::vector<float> exposure, energyTH; std::vector<int> frameID, slots;
    void clear() { evalPT.clear(); state.clear(); state_zero.clear(); exposure.clear(); energyTH.clear(); frameID.clear(); slots.clear(); }
    template <class FrameHessianT, class SlotOf> void push(FrameHessianT* fh, SlotOf& slot_of) {
      const sdso_se3_t T = toAbi(fh->get_worldToCam_evalPT());
      evalPT.insert(evalPT.end(), T.R, T.R + 9); evalPT.insert(evalPT.end(), T.t, T.t + 3);
      for (int i = 0; i < 10; i++) { state.push_back(fh->get_state()[i]); state_zero.push_back(fh->get_state_zero()[i]); }
      exposure.push_back(fh->ab_exposure); energyTH.push_back(fh->frameEnergyTH); frameID.push_back(fh->frameID); slots.push_back(slot_of(fh));
    }
  };
  struct PointCols {
    std::vector<float> u, v, idepth, idepth_zero, color, weights, maxRelBaseline; std::vector<int> host, numGood; std::vector<uint8_t> prior;
    void clear() { u.clear(); v.clear(); idepth.clear(); idepth_zero.clear(); color.clear(); weights.clear(); maxRelBaseline.clear(); host.clear(); numGood.clear(); prior.clear(); }
    template <class PointHessianT> void push(PointHessianT* ph, int host_idx) {
      u.push_back(ph->u); v.push_back(ph->v); idepth.push_back(ph->idepth); idepth_zero.push_back(ph->idepth_zero);
      for (int k = 0; k < 8; k++) { color.push_back(ph->color[k]); weights.push_back(ph->weights[k]); }
      host.push_back(host_idx); prior.push_back(ph->hasDepthPrior ? 1 : 0);
      maxRelBaseline.push_back(ph->maxRelBaseline); numGood.push_back(ph->numGoodResiduals);
    }
  };
  struct ResCols {
    std::vector<int> point, target; std::vector<uint8_t> state, isNew;
    void clear() { point.clear(); target.clear(); state.clear(); isNew.clear(); }
    template <class PointFrameResidualT> void push(int point_idx, int target_idx, PointFrameResidualT* pfr) {
      point.push_back(point_idx); target.push_back(target_idx); state.push_back((uint8_t)pfr->state_state); isNew.push_back(pfr->isNew ? 1 : 0);
    }
  };
  // a vector / an n x m matrix of the reference (Eigen: [i] / (i, j)) from a row-major buffer of the ABI
  template <class V> static void fill_(V& v, const double* src, int n) { for (int i = 0; i < n; i++) v[i] = src[i]; }
  template <class M> static void fill_(M& H, const double* src, int n, int m) { for (int i = 0; i < n; i++) for (int j = 0; j < m; j++) H(i, j) = src[(size_t)i * m + j]; }
  void reindex_() {                                        // points_ / residuals_ -> their index maps
    res_index_.clear(); point_index_.clear();
    for (size_t i = 0; i < residuals_.size(); i++) res_index_[residuals_[i]->data] = (int)i;
    for (size_t i = 0; i < points_.size(); i++) point_index_[points_[i]] = (int)i;
  }
  FrameCols up_frames_; PointCols up_points_; ResCols up_res_;   // upload()'s buffers, kept from call to call
  std::vector<double> HM_, bM_;
  // an SE3 of the reference's type from R, t (Sophus::SE3d(Matrix3d, Vector3d); the prototype only lends its types)
  template <class SE3T>
  static SE3T like(const SE3T& proto, const sdso_se3_t& a) {
    std::decay_t<decltype(proto.rotationMatrix())> R;
    std::decay_t<decltype(proto.translation())> t;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = a.R[i * 3 + j]; t[i] = a.t[i]; }
    return SE3T(R, t);
  }
  std::vector<std::decay_t<decltype(std::declval<EnergyFunctionalT&>().frames[0]->points[0])>> points_;          // EFPoint*
  std::vector<std::decay_t<decltype(std::declval<EnergyFunctionalT&>().frames[0]->points[0]->residualsAll[0])>> residuals_;  // EFResidual*
};

// =================================================================================== accumulators
// AccumulatedTopHessianSSE / AccumulatedSCHessianSSE with the reference's member signatures (AccumulatedTopHessian.h:66-97, :162-169;
// AccumulatedSCHessian.h:66-96, :155-160) over the device window.  The device forms all three accumulations of a linearised state in one
// pass (k_ba_lin_fused / k_ba_accum_top + k_ba_sc_host), so setZero / addPoint<mode> / addPointsInternal<mode> are BOOKKEEPING — which mode
// the caller is accumulating, and for mode 2 (marginalizePointsF, EnergyFunctional.cpp:663-736) which points it passes — and the stitch
// members return the stitched systems of that pass (sdso_ba_get_stitched):
//   top, mode 0 : stitchDouble[MT](H, b, EF, usePrior = false, ..)   accumulateAF_MT  (EnergyFunctional.cpp:212-232)
//   top, mode 1 : stitchDouble[MT](H, b, EF, usePrior = true, ..)    accumulateLF_MT  (:236-254)
//   top, mode 2 : stitchDouble(M, Mb, EF, false, false)               marginalizePointsF (:707): runs sdso_ba_marginalize_points for the collected points
//   bottom      : stitchDouble[MT](H, b, EF, ..)                      accumulateSCF_MT (:256-269) / marginalizePointsF (:708)
// `tid` / `min` / `max` / `stats` / the IndexThreadReduce pointer are accepted and ignored (a GPU backend is free to ignore tid).
template <class BA>
class AccumulatedTopHessianSSE {
 public:
  explicit AccumulatedTopHessianSSE(BA& ba) : ba_(ba) { for (int i = 0; i < 6; i++) { nframes[i] = 0; nres[i] = 0; } }
  int nframes[6];   // NUM_THREADS (util/NumType.h:38)
  int nres[6];
  template <class StatsT = void>
  void setZero(int nFrames, int /*min*/ = 0, int /*max*/ = 1, StatsT* /*stats*/ = 0, int tid = 0) {
    nframes[tid] = nFrames; nres[tid] = 0; mode_ = -1; flagged_.clear();
  }
  template <int mode, class EFPointT, class EFT>
  void addPoint(EFPointT* p, EFT const* /*ef*/, int /*tid*/ = 0) {
    static_assert(mode >= 0 && mode <= 2, "addPoint<mode>: 0 active, 1 linearized, 2 marginalize");
    if (mode_ != -1 && mode_ != mode) throw Error("AccumulatedTopHessianSSE: one mode per setZero");
    mode_ = mode;
    if (mode == 2) flagged_.push_back(p);
  }
  template <int mode, class EFPointT, class EFT, class StatsT = void>
  void addPointsInternal(std::vector<EFPointT*>* points, EFT const* ef, int min = 0, int max = 1, StatsT* /*stats*/ = 0, int tid = 0) {
    for (int i = min; i < max; i++) addPoint<mode>((*points)[i], ef, tid);
  }
  template <class MatXX, class VecX, class EFT>
  void stitchDouble(MatXX& H, VecX& b, EFT const* /*EF*/, bool usePrior, bool /*useDelta*/, int /*tid*/ = 0) { stitch_(H, b, usePrior); }
  template <class RedT, class MatXX, class VecX, class EFT>
  void stitchDoubleMT(RedT* /*red*/, MatXX& H, VecX& b, EFT const* /*EF*/, bool usePrior, bool /*MT*/) { stitch_(H, b, usePrior); }
  const std::vector<const void*>& flagged() const { return flagged_; }

 private:
  template <class MatXX, class VecX> void stitch_(MatXX& H, VecX& b, bool usePrior) {
    if (mode_ == 2) {
      if (usePrior) throw Error("AccumulatedTopHessianSSE: the marginalisation stitch is called without priors (EnergyFunctional.cpp:707)");
      ba_.ensureMarginalizedErased(flagged_);
      ba_.stitchedSystem(0, H, b);
      nres[0] = ba_.lastMargResiduals();
      return;
    }
    // mode 0 is stitched without the priors, mode 1 with them — the only combinations the reference forms (EnergyFunctional.cpp:218, :240)
    const int which = mode_ == 1 ? 1 : 0;
    if (usePrior != (which == 1)) throw Error("AccumulatedTopHessianSSE: accumulateAF_MT stitches without priors, accumulateLF_MT with them");
    ba_.ensureAccumulated();
    ba_.stitchedSystem(which, H, b);
    nres[0] = ba_.countOf(which);
  }
  BA& ba_;
  int mode_ = -1;
  std::vector<const void*> flagged_;
};
template <class BA>
class AccumulatedSCHessianSSE {
 public:
  explicit AccumulatedSCHessianSSE(BA& ba) : ba_(ba) { for (int i = 0; i < 6; i++) nframes[i] = 0; }
  int nframes[6];
  template <class StatsT = void>
  void setZero(int n, int /*min*/ = 0, int /*max*/ = 1, StatsT* /*stats*/ = 0, int tid = 0) { nframes[tid] = n; marg_ = false; }
  template <class EFPointT>
  void addPoint(EFPointT* /*p*/, bool shiftPriorToZero, int /*tid*/ = 0) { if (!shiftPriorToZero) marg_ = true; }   // (false only in marginalizePointsF, :700)
  template <class EFPointT, class StatsT = void>
  void addPointsInternal(std::vector<EFPointT*>* points, bool shiftPriorToZero, int min = 0, int max = 1, StatsT* /*stats*/ = 0, int tid = 0) {
    for (int i = min; i < max; i++) addPoint((*points)[i], shiftPriorToZero, tid);
  }
  template <class MatXX, class VecX, class EFT>
  void stitchDouble(MatXX& H, VecX& b, EFT const* /*EF*/, int /*tid*/ = 0) { stitch_(H, b); }
  template <class RedT, class MatXX, class VecX, class EFT>
  void stitchDoubleMT(RedT* /*red*/, MatXX& H, VecX& b, EFT const* /*EF*/, bool /*MT*/) { stitch_(H, b); }

 private:
  template <class MatXX, class VecX> void stitch_(MatXX& H, VecX& b) {
    if (marg_) ba_.requireMarginalized();     // the top accumulator's stitch (called first, :707-708) ran the device pass
    else ba_.ensureAccumulated();
    ba_.stitchedSystem(2, H, b);
  }
  BA& ba_;
  bool marg_ = false;
};

// =================================================================================== ImmaturePoint
// ImmaturePointStatus ImmaturePoint::traceStereo(FrameHessian* frame, Mat33f K, bool mode_right) for a whole
// vector of points (the callers loop over all immature points: FullSystem.cpp:581-613, :667-725).
template <class ImmaturePointT, class Mat33fT>
inline void traceStereoAll(Device& dev, std::vector<ImmaturePointT*>& pts, int frame_slot, const Mat33fT& K, float baseline, bool mode_right,
                           std::vector<uint8_t>& status_out) {
  const int n = (int)pts.size();
  std::vector<float> us(n), vs(n), imin(n), imins(n), imaxs(n), ids(n), col(n * 8), wgt(n * 8), gH(n * 4), eth(n), q(n), uv(n * 2), itv(n);
  std::vector<uint8_t> lts(n);
  for (int i = 0; i < n; i++) {
    const ImmaturePointT* p = pts[i];
    us[i] = p->u_stereo; vs[i] = p->v_stereo; imin[i] = p->idepth_min; imins[i] = p->idepth_min_stereo; imaxs[i] = p->idepth_max_stereo;
    ids[i] = p->idepth_stereo; eth[i] = p->energyTH; q[i] = p->quality; lts[i] = (uint8_t)p->lastTraceStatus;
    uv[2 * i] = p->lastTraceUV[0]; uv[2 * i + 1] = p->lastTraceUV[1]; itv[i] = p->lastTracePixelInterval;
    for (int k = 0; k < 8; k++) { col[i * 8 + k] = p->color[k]; wgt[i * 8 + k] = p->weights[k]; }
    gH[i * 4 + 0] = p->gradH(0, 0); gH[i * 4 + 1] = p->gradH(0, 1); gH[i * 4 + 2] = p->gradH(1, 0); gH[i * 4 + 3] = p->gradH(1, 1);
  }
  sdso_trace_points_t P{n, us.data(), vs.data(), imin.data(), imins.data(), imaxs.data(), ids.data(), col.data(), wgt.data(), gH.data(), eth.data(),
                        q.data(), lts.data(), uv.data(), itv.data()};
  const float K4[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
  status_out.assign(n, 0);
  dev.check(sdso_trace_stereo_batch(dev.ctx(), frame_slot, K4, baseline, mode_right ? 1 : 0, &P, status_out.data()), "sdso_trace_stereo_batch");
  for (int i = 0; i < n; i++) {
    ImmaturePointT* p = pts[i];
    p->idepth_min_stereo = imins[i]; p->idepth_max_stereo = imaxs[i]; p->idepth_stereo = ids[i]; p->quality = q[i];
    p->lastTraceStatus = static_cast<decltype(p->lastTraceStatus)>(lts[i]);
    p->lastTraceUV[0] = uv[2 * i]; p->lastTraceUV[1] = uv[2 * i + 1]; p->lastTracePixelInterval = itv[i];
  }
}

// The member itself, ONE point (ImmaturePoint.h:89): `ImmaturePointStatus ImmaturePoint::traceStereo(FrameHessian* frame, Mat33f K,
// bool mode_right)` becomes `return sdso_shim::traceStereo(dev, this, slot_of(frame), K, baseline, mode_right);` — same state changes on
// the point, same return value.  A launch per point: the callers' loops (FullSystem.cpp:581-613, :667-725) want traceStereoAll.
template <class ImmaturePointT, class Mat33fT>
inline auto traceStereo(Device& dev, ImmaturePointT* p, int frame_slot, const Mat33fT& K, float baseline, bool mode_right) -> decltype(p->lastTraceStatus) {
  std::vector<ImmaturePointT*> one{p};
  std::vector<uint8_t> st;
  traceStereoAll(dev, one, frame_slot, K, baseline, mode_right, st);
  return static_cast<decltype(p->lastTraceStatus)>(st[0]);
}

// =================================================================================== per-keyframe steps
// PixelSelector (src/FullSystem/PixelSelector2.h): int makeMaps(const FrameHessian* fh, float* map_out, float density,
// int recursionsLeft = 1, bool plot = false, float thFactor = 1); currentPotential is the public member the callers reset.
class PixelSelector {
 public:
  explicit PixelSelector(Device& dev) : dev_(dev) {}
  int currentPotential = 3;
  int makeMaps(int frame_slot, float* map_out, float density, int recursionsLeft = 1, bool /*plot*/ = false, float thFactor = 1) {
    int n = 0;
    dev_.check(sdso_pixel_select(dev_.ctx(), frame_slot, density, recursionsLeft, thFactor, &currentPotential, map_out, &n), "sdso_pixel_select");
    return n;
  }

 private:
  Device& dev_;
};

// ImmaturePoint::traceOn for all immature points of all host keyframes in the newest frame (FullSystem::traceNewCoarseKey / NonKey,
// FullSystem.cpp:632-790).  geom[h] = {KRKi, Kt, aff} of host h as computed at :654-665; host_of[i] selects it.
template <class ImmaturePointT>
inline void traceOnAll(Device& dev, std::vector<ImmaturePointT*>& pts, const std::vector<int>& host_of, const std::vector<sdso_trace_geom_t>& geom,
                       int frame_slot, std::vector<uint8_t>& status_out) {
  const int n = (int)pts.size();
  std::vector<float> us(n), vs(n), imin(n), imax(n), col(n * 8), wgt(n * 8), gH(n * 4), eth(n), q(n), uv(n * 2), itv(n);
  std::vector<uint8_t> lts(n);
  for (int i = 0; i < n; i++) {
    const ImmaturePointT* p = pts[i];
    us[i] = p->u; vs[i] = p->v; imin[i] = p->idepth_min; imax[i] = p->idepth_max; eth[i] = p->energyTH; q[i] = p->quality;
    lts[i] = (uint8_t)p->lastTraceStatus; uv[2 * i] = p->lastTraceUV[0]; uv[2 * i + 1] = p->lastTraceUV[1]; itv[i] = p->lastTracePixelInterval;
    for (int k = 0; k < 8; k++) { col[i * 8 + k] = p->color[k]; wgt[i * 8 + k] = p->weights[k]; }
    gH[i * 4 + 0] = p->gradH(0, 0); gH[i * 4 + 1] = p->gradH(0, 1); gH[i * 4 + 2] = p->gradH(1, 0); gH[i * 4 + 3] = p->gradH(1, 1);
  }
  sdso_trace_points_t P{n, us.data(), vs.data(), nullptr, imin.data(), imax.data(), nullptr, col.data(), wgt.data(), gH.data(), eth.data(),
                        q.data(), lts.data(), uv.data(), itv.data()};
  status_out.assign(n, 0);
  dev.check(sdso_trace_on_batch(dev.ctx(), frame_slot, (int)geom.size(), geom.data(), host_of.data(), &P, status_out.data()), "sdso_trace_on_batch");
  for (int i = 0; i < n; i++) {
    ImmaturePointT* p = pts[i];
    p->idepth_min = imin[i]; p->idepth_max = imax[i]; p->quality = q[i];
    p->lastTraceStatus = static_cast<decltype(p->lastTraceStatus)>(lts[i]);
    p->lastTraceUV[0] = uv[2 * i]; p->lastTraceUV[1] = uv[2 * i + 1]; p->lastTracePixelInterval = itv[i];
  }
}

// The member itself, ONE point (ImmaturePoint.h:90): `ImmaturePointStatus ImmaturePoint::traceOn(FrameHessian* frame, Mat33f
// hostToFrame_KRKi, Vec3f hostToFrame_Kt, Vec2f hostToFrame_affine, CalibHessian* HCalib, bool debugPrint)` becomes
// `return sdso_shim::traceOn(dev, this, slot_of(frame), KRKi, Kt, aff);` (HCalib is not read by the DSO-native body; debugPrint prints).
template <class ImmaturePointT, class Mat33fT, class Vec3fT, class Vec2fT>
inline auto traceOn(Device& dev, ImmaturePointT* p, int frame_slot, const Mat33fT& hostToFrame_KRKi, const Vec3fT& hostToFrame_Kt,
                    const Vec2fT& hostToFrame_affine) -> decltype(p->lastTraceStatus) {
  sdso_trace_geom_t g;
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) g.KRKi[r * 3 + c] = hostToFrame_KRKi(r, c);
  for (int r = 0; r < 3; r++) g.Kt[r] = hostToFrame_Kt[r];
  g.aff[0] = hostToFrame_affine[0]; g.aff[1] = hostToFrame_affine[1];
  std::vector<ImmaturePointT*> one{p};
  std::vector<uint8_t> st;
  traceOnAll(dev, one, std::vector<int>{0}, std::vector<sdso_trace_geom_t>{g}, frame_slot, st);
  return static_cast<decltype(p->lastTraceStatus)>(st[0]);
}

// =================================================================================== CoarseDistanceMap / activatePointsMT STEP 1-2
// class CoarseDistanceMap (FullSystem/CoarseTracker.h:165-197) with the members its caller (FullSystem::activatePointsMT,
// FullSystem.cpp:823-902) touches: makeK(CalibHessian*), makeDistanceMap(frameHessians, frame), addIntoDistFinal(u, v),
// fwdWarpedIDDistFinal, K[], Ki[].  The map itself lives on the device (one per Device); fwdWarpedIDDistFinal is a host copy that
// distFinal() refreshes on demand.  Mat33fT / Vec3fT are the reference's Eigen float types (element access (i, j) / [i]; an
// `inverse()` member is used where the type has one).  The float products K[1] * R * Ki[0] and K[1] * t are formed here, row times
// column summed left to right.
namespace detail {
template <class M> inline auto inverse33(const M& m, int) -> decltype(m.inverse()) { return m.inverse(); }
template <class M> inline M inverse33(const M& m, long) {          // cofactors times 1 / det, in the matrix's own scalar type
  using S = typename std::decay<decltype(m(0, 0))>::type;
  M r;
  const S c00 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), c10 = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), c20 = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0);
  const S id = S(1) / (c00 * m(0, 0) + c10 * m(0, 1) + c20 * m(0, 2));
  r(0, 0) = c00 * id; r(1, 0) = c10 * id; r(2, 0) = c20 * id;
  r(0, 1) = (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * id; r(1, 1) = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * id; r(2, 1) = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * id;
  r(0, 2) = (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * id; r(1, 2) = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * id; r(2, 2) = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * id;
  return r;
}
// a new ImmaturePoint object whose members the caller fills in: the stand-in types are default-constructible; the reference's class
// only has its two pixel constructors (ImmaturePoint.h:85-86), so the int one is used, which reads host->dI on the host and whose
// results are then overwritten
template <class P, class FrameHessianT, class CalibHessianT>
inline P* newImmaturePoint(std::true_type, float, float, FrameHessianT*, float, CalibHessianT*) { return new P(); }
template <class P, class FrameHessianT, class CalibHessianT>
inline P* newImmaturePoint(std::false_type, float u, float v, FrameHessianT* host, float type, CalibHessianT* HCalib) { return new P((int)u, (int)v, host, type, HCalib); }
}  // namespace detail

template <class Mat33fT>
class CoarseDistanceMap {
 public:
  CoarseDistanceMap(Device& dev, int ww, int hh) : dev_(dev), buf_((size_t)(ww / 2) * (hh / 2), 1000.f) {
    fwdWarpedIDDistFinal = buf_.data();
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) w[l] = h[l] = 0;
  }
  // makeK(CalibHessian*) — CoarseTracker.cpp:1374-1402 (pyrLevelsUsed and wG[0] / hG[0] are globals in the reference)
  template <class CalibHessianT>
  void makeK(CalibHessianT* HCalib, int pyrLevelsUsed, int wG0, int hG0) {
    w[0] = wG0; h[0] = hG0;
    fx[0] = HCalib->fxl(); fy[0] = HCalib->fyl(); cx[0] = HCalib->cxl(); cy[0] = HCalib->cyl();
    for (int level = 1; level < pyrLevelsUsed; ++level) {
      w[level] = w[0] >> level; h[level] = h[0] >> level;
      fx[level] = fx[level - 1] * 0.5; fy[level] = fy[level - 1] * 0.5;
      cx[level] = (cx[0] + 0.5) / ((int)1 << level) - 0.5;
      cy[level] = (cy[0] + 0.5) / ((int)1 << level) - 0.5;
    }
    for (int level = 0; level < pyrLevelsUsed; ++level) {
      Mat33fT& k = K[level];
      k(0, 0) = fx[level]; k(0, 1) = 0; k(0, 2) = cx[level]; k(1, 0) = 0; k(1, 1) = fy[level]; k(1, 2) = cy[level]; k(2, 0) = 0; k(2, 1) = 0; k(2, 2) = 1;
      Ki[level] = detail::inverse33(k, 0);
      fxi[level] = Ki[level](0, 0); fyi[level] = Ki[level](1, 1); cxi[level] = Ki[level](0, 2); cyi[level] = Ki[level](1, 2);
    }
  }
  // KRKi = K[1] * fhToNew.rotationMatrix().cast<float>() * Ki[0], Kt = K[1] * fhToNew.translation().cast<float>() with
  // fhToNew = frame->PRE_worldToCam * fh->PRE_camToWorld (CoarseTracker.cpp:1232-1236, FullSystem.cpp:840-842)
  template <class FrameHessianT>
  sdso_distmap_geom_t geomOf(const FrameHessianT* fh, const FrameHessianT* frame) const {
    const auto fhToNew = frame->PRE_worldToCam * fh->PRE_camToWorld;
    const auto R = fhToNew.rotationMatrix();
    const auto t = fhToNew.translation();
    float Rf[9], KR[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rf[i * 3 + j] = (float)R(i, j);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) KR[i * 3 + j] = (K[1](i, 0) * Rf[j] + K[1](i, 1) * Rf[3 + j]) + K[1](i, 2) * Rf[6 + j];
    sdso_distmap_geom_t g;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) g.KRKi[i * 3 + j] = (KR[i * 3] * Ki[0](0, j) + KR[i * 3 + 1] * Ki[0](1, j)) + KR[i * 3 + 2] * Ki[0](2, j);
    for (int i = 0; i < 3; i++) g.Kt[i] = (K[1](i, 0) * (float)t[0] + K[1](i, 1) * (float)t[1]) + K[1](i, 2) * (float)t[2];
    return g;
  }
  // makeDistanceMap(std::vector<FrameHessian*> frameHessians, FrameHessian* frame) — CoarseTracker.cpp:1216-1255
  template <class FrameHessianT>
  void makeDistanceMap(std::vector<FrameHessianT*> frameHessians, FrameHessianT* frame) {
    std::vector<sdso_distmap_geom_t> geom;
    std::vector<int> pg;
    std::vector<float> u, v, id;
    for (FrameHessianT* fh : frameHessians) {
      if (frame == fh) continue;
      geom.push_back(geomOf(fh, frame));
      for (auto* ph : fh->pointHessians) { pg.push_back((int)geom.size() - 1); u.push_back(ph->u); v.push_back(ph->v); id.push_back(ph->idepth_scaled); }
    }
    dev_.check(sdso_distmap_make(dev_.ctx(), w[0], h[0], (int)geom.size(), geom.data(), (int)u.size(), pg.data(), u.data(), v.data(), id.data(), &numItems),
               "sdso_distmap_make");
    stale_ = true;
  }
  // The same on the points of the device-resident window of `ba` (sdso_distmap_make_from_window): u, v and the current idepth of every
  // active point are read where they lie, only the geometries travel.  frameHessians must be the frames of that window (each with its
  // efFrame); `frame` itself, when it is already part of the window, contributes nothing (:1232).
  template <class WindowedBAT, class FrameHessianT>
  void makeDistanceMap(WindowedBAT& ba, std::vector<FrameHessianT*> frameHessians, FrameHessianT* frame) {
    const int nf = ba.frameCount();
    std::vector<sdso_distmap_geom_t> geom((size_t)nf);
    std::vector<uint8_t> skip((size_t)nf, 1);             // a window frame the caller does not name contributes nothing
    for (FrameHessianT* fh : frameHessians) {
      if (frame == fh) continue;
      const int k = ba.frameIndex(fh->efFrame);
      if (k < 0) throw Error("makeDistanceMap: a frame is not part of the device window");
      geom[(size_t)k] = geomOf(fh, frame);
      skip[(size_t)k] = 0;
    }
    dev_.check(sdso_distmap_make_from_window(dev_.ctx(), ba.windowId(), w[0], h[0], geom.data(), skip.data(), &numItems), "sdso_distmap_make_from_window");
    stale_ = true;
  }
  // addIntoDistFinal(int u, int v) — CoarseTracker.cpp:1366-1372
  void addIntoDistFinal(int u, int v) {
    if (w[0] == 0) return;
    dev_.check(sdso_distmap_add(dev_.ctx(), 1, &u, &v), "sdso_distmap_add");
    stale_ = true;
  }
  // the host copy of the map, fetched when the device's has changed since the last call
  float* distFinal() {
    if (stale_) { dev_.check(sdso_distmap_get(dev_.ctx(), buf_.data()), "sdso_distmap_get"); stale_ = false; }
    return fwdWarpedIDDistFinal;
  }
  void markStale() { stale_ = true; }
  Device& device() { return dev_; }

  float* fwdWarpedIDDistFinal;
  Mat33fT K[SDSO_PYR_LEVELS];
  Mat33fT Ki[SDSO_PYR_LEVELS];
  float fx[SDSO_PYR_LEVELS], fy[SDSO_PYR_LEVELS], fxi[SDSO_PYR_LEVELS], fyi[SDSO_PYR_LEVELS];
  float cx[SDSO_PYR_LEVELS], cy[SDSO_PYR_LEVELS], cxi[SDSO_PYR_LEVELS], cyi[SDSO_PYR_LEVELS];
  int w[SDSO_PYR_LEVELS], h[SDSO_PYR_LEVELS];
  int numItems = 0;                                   // bfsNum handed to growDistBFS by the last makeDistanceMap

 private:
  Device& dev_;
  std::vector<float> buf_;
  bool stale_ = false;
};

// activatePointsMT STEP 1 (FullSystem.cpp:798-817): `float currentMinActDist` moved by double literals
inline void updateMinActDist(float& currentMinActDist, int nPoints, float setting_desiredPointDensity) {
  if (nPoints < setting_desiredPointDensity * 0.66) currentMinActDist -= 0.8;
  if (nPoints < setting_desiredPointDensity * 0.8) currentMinActDist -= 0.5;
  else if (nPoints < setting_desiredPointDensity * 0.9) currentMinActDist -= 0.2;
  else if (nPoints < setting_desiredPointDensity) currentMinActDist -= 0.1;
  if (nPoints > setting_desiredPointDensity * 1.5) currentMinActDist += 0.8;
  if (nPoints > setting_desiredPointDensity * 1.3) currentMinActDist += 0.5;
  if (nPoints > setting_desiredPointDensity * 1.15) currentMinActDist += 0.2;
  if (nPoints > setting_desiredPointDensity) currentMinActDist += 0.1;
  if (currentMinActDist < 0) currentMinActDist = 0;
  if (currentMinActDist > 4) currentMinActDist = 4;
}

// activatePointsMT STEP 2 (FullSystem.cpp:837-902) over the callers' immaturePoints vectors, after coarseDistanceMap->makeDistanceMap:
// every candidate gets idxInImmaturePoints, the deleted ones are `delete`d and their entry is set to 0 exactly where the reference
// does it, the selected ones come back in toOptimize order; the map on the device has been re-grown around each of them.
template <class CoarseDistanceMapT, class FrameHessianT>
inline auto selectPointsToActivate(CoarseDistanceMapT& cdm, std::vector<FrameHessianT*>& frameHessians, float currentMinActDist, float setting_minTraceQuality)
    -> std::vector<typename std::remove_reference<decltype(*frameHessians[0]->immaturePoints[0])>::type*> {
  using ImmaturePointT = typename std::remove_reference<decltype(*frameHessians[0]->immaturePoints[0])>::type;
  std::vector<ImmaturePointT*> toOptimize;
  toOptimize.reserve(20000);
  FrameHessianT* newestHs = frameHessians.back();
  std::vector<sdso_distmap_geom_t> geom;
  std::vector<uint8_t> flagged, st;
  std::vector<int> pg;
  std::vector<float> u, v, imin, imax, q, itv, ty;
  for (FrameHessianT* host : frameHessians) {
    if (host == newestHs) continue;
    geom.push_back(cdm.geomOf(host, newestHs));
    flagged.push_back(host->flaggedForMarginalization ? 1 : 0);
    for (unsigned int i = 0; i < host->immaturePoints.size(); i += 1) {
      ImmaturePointT* ph = host->immaturePoints[i];
      ph->idxInImmaturePoints = i;
      pg.push_back((int)geom.size() - 1); u.push_back(ph->u); v.push_back(ph->v); imin.push_back(ph->idepth_min); imax.push_back(ph->idepth_max);
      q.push_back(ph->quality); itv.push_back(ph->lastTracePixelInterval); st.push_back((uint8_t)ph->lastTraceStatus); ty.push_back(ph->my_type);
    }
  }
  const int n = (int)u.size();
  std::vector<uint8_t> decision(n);
  sdso_activate_select_t S{cdm.w[0], cdm.h[0], (int)geom.size(), geom.data(), flagged.data(), n, pg.data(), u.data(), v.data(), imin.data(), imax.data(),
                           q.data(), itv.data(), st.data(), ty.data(), currentMinActDist, setting_minTraceQuality};
  int n_selected = 0;
  cdm.device().check(sdso_activate_select(cdm.device().ctx(), &S, decision.data(), nullptr, nullptr, &n_selected), "sdso_activate_select");
  cdm.markStale();
  int k = 0;
  for (FrameHessianT* host : frameHessians) {
    if (host == newestHs) continue;
    for (unsigned int i = 0; i < host->immaturePoints.size(); i += 1, k++) {
      ImmaturePointT* ph = host->immaturePoints[i];
      if (decision[k] == 1) { delete ph; host->immaturePoints[i] = 0; }
      else if (decision[k] == 2) toOptimize.push_back(ph);
    }
  }
  return toOptimize;
}

// EnergyFunctional::marginalizeFrame's algebra (EnergyFunctional.cpp:554-660) on plain row-major arrays
inline void marginalizeFrame(int nFrames, int idx, const double* prior8, const double* delta_prior8, std::vector<double>& HM, std::vector<double>& bM) {
  const int m = 8 * (nFrames - 1) + 4;
  std::vector<double> Ho((size_t)m * m), bo(m);
  if (sdso_ba_marginalize_frame(nFrames, idx, prior8, delta_prior8, HM.data(), bM.data(), Ho.data(), bo.data()) != SDSO_OK)
    throw Error("sdso_ba_marginalize_frame: bad arguments");
  HM.swap(Ho); bM.swap(bo);
}

// =================================================================================== the device-resident immature points
// FullSystem::makeNewTraces (FullSystem.cpp:1600-1629), traceNewCoarseNonKey (:632-742) and traceNewCoarseKey (:745-781) with the
// reference's signatures, on the set the library keeps on the device (sdso_imm_*): the three bodies no longer touch
// host->immaturePoints.  The object stands for the FullSystem members the bodies read: Hcalib, frameHessians, pixelSelector,
// setting_desiredImmatureDensity and the stereo baseline.  slot_of(frame) is the frame's pyramid slot on the device; a keyframe's slot
// is also its host_id in the set.  activatePointsMT runs STEP 2-5 on the set and returns the activated records; upload(host) installs
// host->immaturePoints as the host's group.  stereoMatch(fh, fh_right, idepthMap) is the loop of FullSystem::stereoMatch (:579-613) on
// fh's group.  download(host) rebuilds host->immaturePoints from the set (what the older activation path reads, and a caller who wants
// the objects); remove(host, flags) is STEP 5 for the entries STEP 2 / STEP 4 set to 0; release(host) goes where the reference deletes a
// marginalized frame's immature points (and before stereoMatch deletes its temporary frame).  A frame of frameHessians without points in
// the set is not traced, like the reference's empty loop.  The benchmark-only and debug branches of the three functions are not mirrored.
// Mat33fT is the reference's Eigen float matrix type (element access (i, j)); products are formed row times column, summed left to right.
template <class FrameHessianT, class CalibHessianT, class Mat33fT>
class ImmaturePoints {
 public:
  using ImmaturePointT = typename std::remove_pointer<typename std::remove_reference<decltype(std::declval<FrameHessianT>().immaturePoints[0])>::type>::type;
  ImmaturePoints(Device& dev, PixelSelector& pixelSelector, CalibHessianT& Hcalib, std::vector<FrameHessianT*>& frameHessians,
                 std::function<int(const FrameHessianT*)> slot_of, float baseline, float setting_desiredImmatureDensity)
      : dev_(dev), sel_(pixelSelector), Hcalib_(Hcalib), frameHessians_(frameHessians), slot_of_(std::move(slot_of)), baseline_(baseline),
        density_(setting_desiredImmatureDensity) {}

  // void FullSystem::makeNewTraces(FrameHessian* newFrame, FrameHessian* newFrameRight, float* gtDepth): the selection map stays on the
  // device between makeMaps and the constructor loop.  Only enqueues after makeMaps; returns makeMaps' numPointsTotal.
  int makeNewTraces(FrameHessianT* newFrame, FrameHessianT* /*newFrameRight*/, float* /*gtDepth*/) {
    const int slot = slot_of_(newFrame);
    const int numPointsTotal = sel_.makeMaps(slot, nullptr, density_);
    dev_.check(sdso_imm_add_frame(dev_.ctx(), slot, slot, nullptr, nullptr), "sdso_imm_add_frame");
    return numPointsTotal;
  }
  void traceNewCoarseNonKey(FrameHessianT* fh, FrameHessianT* fh_right) { trace_(fh, fh_right); }
  void traceNewCoarseKey(FrameHessianT* fh, FrameHessianT* /*fh_right*/) { trace_(fh, nullptr); }

  // the geometry of :654-665 for one host
  sdso_imm_geom_t geomOf(const FrameHessianT* host, const FrameHessianT* fh) const {
    Mat33fT K, Ki;
    makeK(K, Ki);
    const auto hostToNew = fh->PRE_worldToCam * host->PRE_camToWorld;
    const auto R = hostToNew.rotationMatrix();
    const auto t = hostToNew.translation();
    const auto Ri = detail::inverse33(R, 0);   // hostToNew.rotationMatrix().inverse(), in double (:658)
    float Rf[9], Rif[9], KR[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { Rf[i * 3 + j] = (float)R(i, j); Rif[i * 3 + j] = (float)Ri(i, j); }
    sdso_imm_geom_t g;
    g.host_id = slot_of_(host);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) KR[i * 3 + j] = (K(i, 0) * Rf[j] + K(i, 1) * Rf[3 + j]) + K(i, 2) * Rf[6 + j];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) g.KRKi[i * 3 + j] = (KR[i * 3] * Ki(0, j) + KR[i * 3 + 1] * Ki(1, j)) + KR[i * 3 + 2] * Ki(2, j);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) g.KRi[i * 3 + j] = (K(i, 0) * Rif[j] + K(i, 1) * Rif[3 + j]) + K(i, 2) * Rif[6 + j];
    for (int i = 0; i < 3; i++) { g.t[i] = (float)t[i]; g.Kt[i] = (K(i, 0) * (float)t[0] + K(i, 1) * (float)t[1]) + K(i, 2) * (float)t[2]; }
    using AffLightT = typename std::decay<decltype(host->aff_g2l())>::type;
    const auto aff = AffLightT::fromToVecExposure(host->ab_exposure, fh->ab_exposure, host->aff_g2l(), fh->aff_g2l());
    g.aff[0] = (float)aff[0]; g.aff[1] = (float)aff[1];
    return g;
  }
  int count(const FrameHessianT* host) const {
    int n = 0;
    dev_.check(sdso_imm_count(dev_.ctx(), slot_of_(host), &n), "sdso_imm_count");
    return n;
  }
  // host->immaturePoints <- the set's points of this host, in the set's order (the old objects are deleted)
  void download(FrameHessianT* host) {
    const int n = count(host);
    std::vector<float> us(n), vs(n), ty(n), imin(n), imax(n), col(n * 8), wgt(n * 8), gH(n * 4), eth(n), q(n), uv(n * 2), itv(n);
    std::vector<uint8_t> lts(n);
    sdso_trace_points_t P{n, us.data(), vs.data(), nullptr, imin.data(), imax.data(), nullptr, col.data(), wgt.data(), gH.data(), eth.data(),
                          q.data(), lts.data(), uv.data(), itv.data()};
    if (n) dev_.check(sdso_imm_get(dev_.ctx(), slot_of_(host), &P, ty.data()), "sdso_imm_get");
    for (ImmaturePointT* p : host->immaturePoints) delete p;
    host->immaturePoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
      ImmaturePointT* p = detail::newImmaturePoint<ImmaturePointT>(std::is_default_constructible<ImmaturePointT>(), us[i], vs[i], host, ty[i], &Hcalib_);
      p->host = host; p->idxInImmaturePoints = i;
      p->u = us[i]; p->v = vs[i]; p->my_type = ty[i]; p->idepth_min = imin[i]; p->idepth_max = imax[i]; p->quality = q[i]; p->energyTH = eth[i];
      p->lastTraceStatus = static_cast<decltype(p->lastTraceStatus)>(lts[i]);
      p->lastTraceUV[0] = uv[2 * i]; p->lastTraceUV[1] = uv[2 * i + 1]; p->lastTracePixelInterval = itv[i];
      for (int k = 0; k < 8; k++) { p->color[k] = col[i * 8 + k]; p->weights[k] = wgt[i * 8 + k]; }
      p->gradH(0, 0) = gH[i * 4 + 0]; p->gradH(0, 1) = gH[i * 4 + 1]; p->gradH(1, 0) = gH[i * 4 + 2]; p->gradH(1, 1) = gH[i * 4 + 3];
      host->immaturePoints[i] = p;
    }
  }
  // The loop of FullSystem::stereoMatch (FullSystem.cpp:579-613) after makeNewTraces(fh, fh_right, 0): every point of fh traced into
  // fh_right and back, the accept rule of :601 with the reference's depth < 70, and for every accepted point idepth_stereo, idepth_min,
  // idepth_max at (float*)(idepthMap.data + int(v) * idepthMap.step) + (int)u * 3.  No other pixel is touched, as in the reference; returns
  // `counter`.  MatT: the reference's cv::Mat (CV_32FC3), or anything with `unsigned char* data` and `size_t step`.  The traces and the
  // rule run on the device (sdso_imm_stereo_match); 13 bytes per point come back, and u, v (8 more) for the pixel.  fh->immaturePoints is
  // not touched and the group stays in the set: release(fh) goes where the reference deletes fh.
  template <class MatT>
  int stereoMatch(FrameHessianT* fh, FrameHessianT* fh_right, MatT& idepthMap) {
    const int n = count(fh);
    std::vector<uint8_t> accepted(n);
    std::vector<float> idepth((size_t)n * 3), us(n), vs(n);
    sdso_imm_match_out_t O{accepted.data(), idepth.data(), nullptr, nullptr, nullptr};
    const float K4[4] = {Hcalib_.fxl(), Hcalib_.fyl(), Hcalib_.cxl(), Hcalib_.cyl()};   // K of :569-573
    int counts[SDSO_IMM_MATCH_NCOUNTS];
    dev_.check(sdso_imm_stereo_match(dev_.ctx(), slot_of_(fh), slot_of_(fh), slot_of_(fh_right), K4, baseline_, 70.f, 0, &O, counts), "sdso_imm_stereo_match");
    sdso_trace_points_t P{};
    P.n = n; P.u_stereo = us.data(); P.v_stereo = vs.data();
    if (n) dev_.check(sdso_imm_get(dev_.ctx(), slot_of_(fh), &P, nullptr), "sdso_imm_get");
    unsigned char* idepthMapPtr = idepthMap.data;
    int counter = 0;
    for (int i = 0; i < n; i++)
      if (accepted[i]) {
        float* px = (float*)(idepthMapPtr + int(vs[i]) * idepthMap.step) + (int)us[i] * 3;
        px[0] = idepth[(size_t)i * 3]; px[1] = idepth[(size_t)i * 3 + 1]; px[2] = idepth[(size_t)i * 3 + 2];
        counter++;
      }
    return counter;
  }
  // STEP 5 (:948-957) on the device: flags[i] != 0 where STEP 2 / STEP 4 set host->immaturePoints[i] = 0
  void remove(const FrameHessianT* host, const std::vector<uint8_t>& flags) {
    dev_.check(sdso_imm_remove(dev_.ctx(), slot_of_(host), (int)flags.size(), flags.data()), "sdso_imm_remove");
  }
  void release(const FrameHessianT* host) { dev_.check(sdso_imm_release_host(dev_.ctx(), slot_of_(host)), "sdso_imm_release_host"); }

  // the set's points of this host <- host->immaturePoints, in the vector's order: the counterpart of download, for a caller that switches
  // to the resident set in mid-run or made the points on the host (the host must not have points in the set: release first)
  void upload(const FrameHessianT* host, int w, int h) {
    const int n = (int)host->immaturePoints.size();
    std::vector<float> us(n), vs(n), ty(n), imin(n), imax(n), col(n * 8), wgt(n * 8), gH(n * 4), eth(n), q(n), uv(n * 2), itv(n);
    std::vector<uint8_t> lts(n);
    for (int i = 0; i < n; i++) {
      const ImmaturePointT* p = host->immaturePoints[i];
      us[i] = p->u; vs[i] = p->v; ty[i] = p->my_type; imin[i] = p->idepth_min; imax[i] = p->idepth_max; q[i] = p->quality; eth[i] = p->energyTH;
      lts[i] = (uint8_t)p->lastTraceStatus; uv[2 * i] = p->lastTraceUV[0]; uv[2 * i + 1] = p->lastTraceUV[1]; itv[i] = p->lastTracePixelInterval;
      for (int k = 0; k < 8; k++) { col[i * 8 + k] = p->color[k]; wgt[i * 8 + k] = p->weights[k]; }
      gH[i * 4 + 0] = p->gradH(0, 0); gH[i * 4 + 1] = p->gradH(0, 1); gH[i * 4 + 2] = p->gradH(1, 0); gH[i * 4 + 3] = p->gradH(1, 1);
    }
    sdso_trace_points_t P{n, us.data(), vs.data(), nullptr, imin.data(), imax.data(), nullptr, col.data(), wgt.data(), gH.data(), eth.data(),
                          q.data(), lts.data(), uv.data(), itv.data()};
    dev_.check(sdso_imm_put_host(dev_.ctx(), slot_of_(host), w, h, &P, ty.data()), "sdso_imm_put_host");
  }

  // One entry of toOptimize after STEP 3: what optimizeImmaturePoint returned for it (status 1 = a PointHessian, 0 = null, -1 =
  // (PointHessian*)-1; FullSystemOptPoint.cpp:52-238) and the members PointHessian::PointHessian(const ImmaturePoint*, ...) copies
  // (HessianBlocks.cpp:35-70).  res_state[f] is the final ResState of the residual to frameHessians[f] (0 IN, 1 OOB, 2 OUTLIER; 255 for
  // the host itself and for a status-0 exit).
  struct Activated {
    FrameHessianT* host;
    int idxInImmaturePoints;       // in the host's group BEFORE this call's removal
    int status;
    float idepth;                  // currentIdepth: setIdepthZero / setIdepth (:208-209)
    uint8_t res_state[SDSO_IMM_MAX_HOSTS];
    float u, v, my_type, idepth_min, idepth_max, energyTH, color[8], weights[8];
    int lastTraceStatus;
  };
  // FullSystem::activatePointsMT STEP 2-5 (FullSystem.cpp:837-957) on the set, after coarseDistanceMap->makeDistanceMap(frameHessians,
  // newestHs): no ImmaturePoint object is built.  Reads what the reference's body reads — cdm.geomOf (:841-842),
  // host->targetPrecalc[target->idx].PRE_RTll / PRE_tTll / PRE_aff_mode (ImmaturePoint.cpp:897-901), flaggedForMarginalization, the
  // frames' pyramid slots — and returns the entries of toOptimize.  The caller's STEP 3 tail and STEP 4 become one loop over them: for
  // status 1 `new PointHessian`, setIdepthZero, the PointFrameResiduals of the IN targets, lastResiduals[0/1], ef->insertPoint /
  // insertResidual (FullSystemOptPoint.cpp:196-237, FullSystem.cpp:923-933).  The removal of STEP 4 / STEP 5 has already happened in
  // the set; host->immaturePoints is not touched.  minObs: the reference passes 1 (FullSystem.cpp:790).
  template <class CoarseDistanceMapT>
  std::vector<Activated> activatePointsMT(CoarseDistanceMapT& cdm, std::vector<FrameHessianT*>& frameHessians, float currentMinActDist,
                                          float setting_minTraceQuality, int minObs = 1) {
    const int nf = (int)frameHessians.size();
    if (nf < 2 || nf > SDSO_IMM_MAX_HOSTS) throw Error("activatePointsMT: 2..8 frames");
    FrameHessianT* newestHs = frameHessians.back();
    std::vector<int> host_id(nf), slot(nf);
    std::vector<uint8_t> flagged(nf);
    std::vector<sdso_distmap_geom_t> geom;
    std::vector<float> pR((size_t)nf * nf * 9), pt((size_t)nf * nf * 3), pa((size_t)nf * nf * 2);
    for (int f = 0; f < nf; f++) {
      const FrameHessianT* host = frameHessians[f];
      host_id[f] = slot[f] = slot_of_(host);
      flagged[f] = host->flaggedForMarginalization ? 1 : 0;
      if (host != newestHs) geom.push_back(cdm.geomOf(host, newestHs));
      for (int t = 0; t < nf; t++) {
        const auto& pre = host->targetPrecalc[frameHessians[t]->idx];
        const size_t k = (size_t)f * nf + t;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) pR[k * 9 + i * 3 + j] = pre.PRE_RTll(i, j);
        for (int i = 0; i < 3; i++) pt[k * 3 + i] = pre.PRE_tTll[i];
        pa[k * 2] = pre.PRE_aff_mode[0]; pa[k * 2 + 1] = pre.PRE_aff_mode[1];
      }
    }
    sdso_imm_activate_t A{nf, host_id.data(), slot.data(), flagged.data(), geom.data(), pR.data(), pt.data(), pa.data(), cdm.w[0], cdm.h[0],
                          {Hcalib_.fxl(), Hcalib_.fyl(), Hcalib_.cxl(), Hcalib_.cyl()}, minObs, currentMinActDist, setting_minTraceQuality};
    int counts[SDSO_IMM_ACT_NCOUNTS];
    dev_.check(sdso_imm_activate(dev_.ctx(), &A, counts), "sdso_imm_activate");
    cdm.markStale();
    const int n = counts[4];
    std::vector<int> frame(n), index(n);
    std::vector<int8_t> status(n);
    std::vector<uint8_t> rs((size_t)n * nf), lts(n);
    std::vector<float> idepth(n), us(n), vs(n), ty(n), imin(n), imax(n), eth(n), col((size_t)n * 8), wgt((size_t)n * 8);
    sdso_imm_activated_t O{n, nf, frame.data(), index.data(), status.data(), idepth.data(), rs.data(), us.data(), vs.data(), ty.data(), imin.data(), imax.data(),
                           eth.data(), col.data(), wgt.data(), lts.data()};
    dev_.check(sdso_imm_activate_fetch(dev_.ctx(), &O, nullptr), "sdso_imm_activate_fetch");
    std::vector<Activated> out(n);
    for (int p = 0; p < n; p++) {
      Activated& a = out[p];
      a.host = frameHessians[frame[p]]; a.idxInImmaturePoints = index[p]; a.status = status[p]; a.idepth = idepth[p];
      for (int f = 0; f < SDSO_IMM_MAX_HOSTS; f++) a.res_state[f] = f < nf ? rs[(size_t)p * nf + f] : 255;
      a.u = us[p]; a.v = vs[p]; a.my_type = ty[p]; a.idepth_min = imin[p]; a.idepth_max = imax[p]; a.energyTH = eth[p];
      for (int k = 0; k < 8; k++) { a.color[k] = col[(size_t)p * 8 + k]; a.weights[k] = wgt[(size_t)p * 8 + k]; }
      a.lastTraceStatus = lts[p];
    }
    return out;
  }

  // K and K.inverse() of :639-645
  void makeK(Mat33fT& K, Mat33fT& Ki) const {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K(i, j) = i == j ? 1.f : 0.f;
    K(0, 0) = Hcalib_.fxl(); K(1, 1) = Hcalib_.fyl(); K(0, 2) = Hcalib_.cxl(); K(1, 2) = Hcalib_.cyl();
    Ki = detail::inverse33(K, 0);
  }

 private:
  void trace_(FrameHessianT* fh, FrameHessianT* fh_right) {
    Mat33fT K, Ki;
    makeK(K, Ki);
    std::vector<sdso_imm_geom_t> geom;
    // a frame without points in the set (the first frame, pushed by initializeFromInitializer without makeNewTraces, :1487-1500; a
    // keyframe all of whose points are gone) is an empty loop in the reference: it is not named
    for (FrameHessianT* host : frameHessians_)
      if (count(host) > 0) geom.push_back(geomOf(host, fh));
    if (geom.empty()) return;
    const float K4[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    float Ki9[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ki9[i * 3 + j] = Ki(i, j);
    dev_.check(sdso_imm_trace(dev_.ctx(), slot_of_(fh), fh_right ? slot_of_(fh_right) : -1, (int)geom.size(), geom.data(), K4, Ki9, baseline_, nullptr),
               "sdso_imm_trace");
  }
  Device& dev_;
  PixelSelector& sel_;
  CalibHessianT& Hcalib_;
  std::vector<FrameHessianT*>& frameHessians_;
  std::function<int(const FrameHessianT*)> slot_of_;
  float baseline_, density_;
};

// =================================================================================== the stereo initialiser
// class CoarseInitializer (FullSystem/CoarseInitializer.h), the part the stereo fork runs: setFirstStereo (CoarseInitializer.cpp:838-1034,
// called at FullSystem.cpp:1092-1093) and what FullSystem::initializeFromInitializer reads of it (FullSystem.cpp:1487-1597: firstFrame,
// firstRightFrame, thisToNext, numPoints[0], points[0]), on the initialiser state of the Device's ctx (sdso_init_*).  Levels >= 1, makeNN,
// dGrads, setFirst, trackFrame and calcResAndGS are not mirrored: their only reader is the monocular trackFrame, which the fork never calls.
// (ww, hh) is the reference's constructor pair; slot_of(frame) is the frame's pyramid slot on the device, the first frame's with levels
// 0..2 (the selector).  SE3T is the reference's Sophus::SE3d.
template <class FrameHessianT, class CalibHessianT, class SE3T>
class CoarseInitializer {
 public:
  struct Pnt { float u, v, idepth, iR; bool isGood; float my_type, outlierTH; };   // CoarseInitializer.h:38-97, the members setFirstStereo sets
  // One point of STEP 3 (FullSystem.cpp:1533-1573): what PointHessian::PointHessian(const ImmaturePoint*, CalibHessian*) copies
  // (HessianBlocks.cpp:35-68), idepth = the argument of setIdepthScaled and setIdepthZero (:1565-1566), and the index of its Pnt.
  struct Point { int pnt; float u, v, my_type, idepth, idepth_min, idepth_max, energyTH, color[8], weights[8]; };
  CoarseInitializer(Device& dev, int ww, int hh, std::function<int(const FrameHessianT*)> slot_of, float baseline, float setting_outlierTH = 12 * 12)
      : dev_(dev), w_(ww), h_(hh), slot_of_(std::move(slot_of)), baseline_(baseline), outlierTH_(setting_outlierTH) {}

  FrameHessianT* firstFrame = nullptr;        // CoarseInitializer.h:133, :138
  FrameHessianT* firstRightFrame = nullptr;
  SE3T thisToNext;                            // :131
  int frameID = -1;                           // :115, CoarseInitializer.cpp:55
  bool snapped = false;                       // :160
  int snappedAt = 0;                          // :163
  int numPoints[SDSO_PYR_LEVELS] = {};        // :125; [0] alone is set

  // void CoarseInitializer::setFirstStereo(CalibHessian* HCalib, FrameHessian* newFrameHessian, FrameHessian* newFrameHessian_Right).
  // The reference's local `PixelSelector sel(w[0], h[0])` seeds the process's generator and draws w*h values (PixelSelector2.cpp:43-45);
  // the library carries its own copy of that pattern, so the same calls are made here and the process's rand() stream stands where the
  // reference leaves it: the draws of initializeFromInitializer (:1535) follow from there.
  void setFirstStereo(CalibHessianT* HCalib, FrameHessianT* newFrameHessian, FrameHessianT* newFrameHessian_Right) {
    firstFrame = newFrameHessian;
    firstRightFrame = newFrameHessian_Right;
    K_[0] = HCalib->fxl(); K_[1] = HCalib->fyl(); K_[2] = HCalib->cxl(); K_[3] = HCalib->cyl();   // :853-857
    dev_.check(sdso_init_set_first_stereo(dev_.ctx(), slot_of_(firstFrame), slot_of_(firstRightFrame), K_, baseline_, nullptr, &numPoints[0], nullptr),
               "sdso_init_set_first_stereo");
    std::srand(3141592);
    for (int i = 0; i < w_ * h_; i++) std::rand();
    thisToNext = SE3T();                      // :1027-1029
    snapped = false;
    frameID = snappedAt = 0;
  }
  // points[0] (:883-969), one copy from the device
  std::vector<Pnt> points0() const {
    const int n = numPoints[0];
    std::vector<float> u(n), v(n), idepth(n), iR(n), ty(n);
    sdso_init_pnts_t P{n, u.data(), v.data(), idepth.data(), iR.data(), ty.data(), nullptr};
    dev_.check(sdso_init_get_pnts(dev_.ctx(), &P), "sdso_init_get_pnts");
    std::vector<Pnt> out(P.n);
    for (int i = 0; i < P.n; i++) out[i] = Pnt{u[i], v[i], idepth[i], iR[i], true, ty[i], SDSO_PATTERN * outlierTH_};
    return out;
  }
  // STEP 3 of FullSystem::initializeFromInitializer (FullSystem.cpp:1533-1573) with keepPercentage of :1525: one draw of
  // `rand()/(float)RAND_MAX > keepPercentage` per Pnt in order, as :1535 makes them; the constructor, the trace and the filter of
  // :1538-1559 on the device.  Returns the points in push order; the caller's loop body makes `new PointHessian` from each, sets
  // hasDepthPrior and ACTIVE, pushes it to firstFrame->pointHessians and calls ef->insertPoint (:1561-1572).
  std::vector<Point> initializeFromInitializer(float keepPercentage) {
    const int n = numPoints[0];
    std::vector<uint8_t> keep(n);
    for (int i = 0; i < n; i++) keep[i] = std::rand() / (float)RAND_MAX > keepPercentage ? 0 : 1;
    int np = 0;
    dev_.check(sdso_init_from_initializer(dev_.ctx(), keep.data(), &np, nullptr), "sdso_init_from_initializer");
    std::vector<int> pnt(np);
    std::vector<float> u(np), v(np), ty(np), idepth(np), imin(np), imax(np), eth(np), col((size_t)np * 8), wgt((size_t)np * 8);
    sdso_init_points_t P{np, pnt.data(), u.data(), v.data(), ty.data(), idepth.data(), imin.data(), imax.data(), eth.data(), col.data(), wgt.data()};
    dev_.check(sdso_init_get_points(dev_.ctx(), &P), "sdso_init_get_points");
    std::vector<Point> out(P.n);
    for (int i = 0; i < P.n; i++) {
      Point& p = out[i];
      p.pnt = pnt[i]; p.u = u[i]; p.v = v[i]; p.my_type = ty[i]; p.idepth = idepth[i]; p.idepth_min = imin[i]; p.idepth_max = imax[i]; p.energyTH = eth[i];
      for (int k = 0; k < 8; k++) { p.color[k] = col[(size_t)i * 8 + k]; p.weights[k] = wgt[(size_t)i * 8 + k]; }
    }
    return out;
  }

 private:
  Device& dev_;
  int w_, h_;
  std::function<int(const FrameHessianT*)> slot_of_;
  float baseline_, outlierTH_;
  float K_[4] = {0, 0, 0, 0};
};

// =================================================================================== Undistort
// class Undistort (util/Undistort.h:63-104) with the members DatasetReader and main touch: getK, getSize, getOriginalSize, getBl,
// isValid, loadPhotometricCalibration and undistort<T>.  undistort<T> does not return an ImageAndExposure: the undistorted image never
// exists on the host.  It ingests the raw image into a device pyramid slot (Undistort.cpp:398-489 + FrameHessian::makeImages) and
// returns ImageAndExposure::exposure_time; the call only enqueues (sdso_ingest_frame).  Reading the calibration, response and vignette
// files stays with the caller (readFromFile's sscanfs, ImageRW): the class is constructed either from the parsed model parameters or
// from caller-owned remap arrays (the reference's own Undistort::remapX / remapY), and loadPhotometricCalibration takes the tables.
// Mat33T / Vec2iT are the reference's Eigen types (element access (i, j) / [i]).  calib_id names the tables on the device.
template <class Mat33T, class Vec2iT>
class Undistort {
 public:
  // from model parameters: model = SDSO_CAM_*, parsOrg = the 5 or 8 numbers of the first line of the calibration file, out_mode =
  // SDSO_RECTIFY_* (line 3), out_calib = the first four numbers of that line (relative fx fy cx cy; its fifth is unused) when it holds an explicit K, else unused,
  // bl = the baseline (line 5)
  Undistort(Device& dev, int calib_id, int model, const double* parsOrg, int wOrg_, int hOrg_, int w_, int h_, int out_mode, const float* out_calib, float bl_)
      : dev_(dev), calib_(calib_id), wOrg(wOrg_), hOrg(hOrg_), w(w_), h(h_), bl(bl_), remapX_((size_t)w_ * h_), remapY_((size_t)w_ * h_) {
    double k[4];
    int pt = 0;
    if (sdso_undistort_make_remap(model, parsOrg, wOrg, hOrg, w, h, out_mode, out_calib, k, remapX_.data(), remapY_.data(), &pt) != SDSO_OK)
      throw Error("Undistort: the reference exits here (rectification mode, sizes, or makeOptimalK_crop does not converge)");
    passthrough = pt != 0;
    setK_(k);
    valid = true;
  }
  // from caller-owned tables (copied): K = fx fy cx cy of the rectified camera; remapX == nullptr: passthrough
  Undistort(Device& dev, int calib_id, const double K4[4], int wOrg_, int hOrg_, int w_, int h_, const float* remapX, const float* remapY, float bl_)
      : dev_(dev), calib_(calib_id), wOrg(wOrg_), hOrg(hOrg_), w(w_), h(h_), bl(bl_) {
    passthrough = remapX == nullptr;
    if (remapX) { remapX_.assign(remapX, remapX + (size_t)w * h); remapY_.assign(remapY, remapY + (size_t)w * h); }
    setK_(K4);
    valid = true;
  }
  ~Undistort() { if (loaded_) sdso_ingest_calib_release(dev_.ctx(), calib_); }
  Undistort(const Undistort&) = delete;
  Undistort& operator=(const Undistort&) = delete;

  const Mat33T getK() const { return K; }
  const Vec2iT getSize() const { Vec2iT v; v[0] = w; v[1] = h; return v; }
  const Vec2iT getOriginalSize() const { Vec2iT v; v[0] = wOrg; v[1] = hOrg; return v; }
  bool isValid() const { return valid; }
  float getBl() const { return bl; }
  const float* remapX() const { return passthrough ? nullptr : remapX_.data(); }
  const float* remapY() const { return passthrough ? nullptr : remapY_.data(); }

  // loadPhotometricCalibration with the tables instead of the file names: G = PhotometricUndistorter::getG() (256 floats for 8-bit
  // images, 65536 for 16-bit ones; nullptr = no valid calibration), vignetteMapInv = wOrg*hOrg floats or nullptr; the two settings are
  // setting_photometricCalibration and setting_useExposure.  Uploads the tables; they stay on the device until the object goes.
  void loadPhotometricCalibration(int pixel_bytes, const float* G, const float* vignetteMapInv, int setting_photometricCalibration, bool setting_useExposure) {
    dev_.check(sdso_ingest_calib_create(dev_.ctx(), calib_, wOrg, hOrg, w, h, remapX(), remapY(), pixel_bytes, G, vignetteMapInv,
                                        setting_photometricCalibration, setting_useExposure ? 1 : 0), "sdso_ingest_calib_create");
    loaded_ = true;
    pixel_bytes_ = pixel_bytes;
  }

  // undistort<T>(image_raw, exposure, timestamp, factor) into pyramid slot `slot`; MinimalImageT carries data / w / h.  Returns exposure_time.
  template <class MinimalImageT>
  float undistort(const MinimalImageT* image_raw, int slot, float exposure = 0, double /*timestamp*/ = 0, float factor = 1) const {
    check_(image_raw);
    const void* raw[1] = {image_raw->data};
    float out = 0;
    dev_.check(sdso_ingest_frame(dev_.ctx(), calib_, 1, &slot, raw, &exposure, factor, &out), "sdso_ingest_frame");
    return out;
  }
  // the two images of a stereo frame in one call (DatasetReader::getImage for the left and the right reader): one level-0 launch
  template <class MinimalImageT>
  void undistortStereo(const MinimalImageT* left, const MinimalImageT* right, int slot_left, int slot_right, const float exposure[2], float factor, float exposure_out[2]) const {
    check_(left); check_(right);
    const void* raw[2] = {left->data, right->data};
    const int slots[2] = {slot_left, slot_right};
    dev_.check(sdso_ingest_frame(dev_.ctx(), calib_, 2, slots, raw, exposure, factor, exposure_out), "sdso_ingest_frame");
  }

 private:
  template <class MinimalImageT>
  void check_(const MinimalImageT* im) const {
    if (!loaded_) throw Error("Undistort::undistort: loadPhotometricCalibration has not been called");
    if (!im || im->w != wOrg || im->h != hOrg) throw Error("Undistort::undistort: wrong image size");
    if ((int)sizeof(*im->data) != pixel_bytes_) throw Error("Undistort::undistort: pixel type differs from the calibration's");
  }
  void setK_(const double k[4]) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K(i, j) = i == j ? 1.0 : 0.0;
    K(0, 0) = k[0]; K(1, 1) = k[1]; K(0, 2) = k[2]; K(1, 2) = k[3];
  }
  Device& dev_;
  int calib_;
  int wOrg, hOrg, w, h;
  float bl;
  Mat33T K;
  bool valid = false, passthrough = false, loaded_ = false;
  int pixel_bytes_ = 1;
  std::vector<float> remapX_, remapY_;
};

// ---- The device-resident map (sdso_map_*): what FullSystem::makeKeyFrame publishes through publishKeyframes (FullSystem.cpp:1467,
// FullSystemMarginalize.cpp:184) and KeyFrameDisplay turns into vertices and colours.
//
// PointMap::update(ba, frameHessians) — setFromKF's copy of every keyframe's three PointHessian lists, made on the device while the
// window's post-state is valid: call it after ba.flagPointsForRemoval(frameHessians) and before marginalizePointsF / ba.update().
//   active : each frame's pointHessians as the two functions compacted them
//   gone   : the tail each frame's pointHessiansOut / pointHessiansMarginalized has grown by since the previous call (the two sizes are
//            kept per frameID), which is the reference's push order.  A keyframe that joins with lists already filled: note(fh) first,
//            after sdso_map_put of what they hold.
// frameHessians: std::vector<FrameHessian*>-like in window order; of a frame frameID and the three lists are read.  Throws Error when the
// device refuses, and then keeps its sizes as they were.
class PointMap {
 public:
  explicit PointMap(Device& dev) : dev_(dev) {}
  template <class WindowedBAT, class FrameHessians>
  void update(WindowedBAT& ba, FrameHessians& frameHessians) {
    std::vector<int> active, gone;
    std::vector<uint8_t> gone_list;
    std::map<int, Sizes> now = sizes_;
    auto index = [&](const auto* ph) {
      const int i = ph->efPoint ? ba.pointIndexOf(ph->efPoint) : -1;
      if (i < 0) throw Error("PointMap::update: a listed point is not part of the device window (call it before dropPointsF / update())");
      return i;
    };
    for (auto* fh : frameHessians) {
      for (auto* ph : fh->pointHessians) active.push_back(index(ph));
      Sizes& s = now[fh->frameID];
      if (s.out > fh->pointHessiansOut.size() || s.marg > fh->pointHessiansMarginalized.size()) throw Error("PointMap::update: a list of a known frame shrank");
      for (size_t k = s.out; k < fh->pointHessiansOut.size(); k++) { gone.push_back(index(fh->pointHessiansOut[k])); gone_list.push_back(3); }
      for (size_t k = s.marg; k < fh->pointHessiansMarginalized.size(); k++) { gone.push_back(index(fh->pointHessiansMarginalized[k])); gone_list.push_back(2); }
      s.out = fh->pointHessiansOut.size(); s.marg = fh->pointHessiansMarginalized.size();
    }
    sdso_map_update_t U;
    U.n_active = (int)active.size(); U.active = active.data();
    U.n_gone = (int)gone.size(); U.gone = gone.data(); U.gone_list = gone_list.data();
    dev_.check(sdso_map_update(dev_.ctx(), ba.win(), &U), "sdso_map_update");
    sizes_.swap(now);
  }
  template <class FrameHessianT> void note(const FrameHessianT* fh) { sizes_[fh->frameID] = Sizes{fh->pointHessiansOut.size(), fh->pointHessiansMarginalized.size()}; }
  // after the frame's `final = true` publication (FullSystemMarginalize.cpp:184)
  void release(int frameID) { dev_.check(sdso_map_release_keyframe(dev_.ctx(), frameID), "sdso_map_release_keyframe"); sizes_.erase(frameID); }
  // records (16 floats each, sdso_abi.h) of list 1 (active), 2 (marginalised) or 3 (out) of a keyframe
  std::vector<float> records(int frameID, int list) const {
    int c[3] = {0, 0, 0};
    dev_.check(sdso_map_counts(dev_.ctx(), frameID, c), "sdso_map_counts");
    std::vector<float> r((size_t)c[list - 1] * 16);
    dev_.check(sdso_map_get(dev_.ctx(), frameID, list, r.data()), "sdso_map_get");
    return r;
  }

 private:
  struct Sizes { size_t out = 0, marg = 0; };
  Device& dev_;
  std::map<int, Sizes> sizes_;
};

// KeyFrameDisplay (IOWrapper/Pangolin/KeyFrameDisplay.h) on the map, with the reference's member names and signatures.
//   setFromKF(fh, HCalib)   notes the frameID, the immature group (immGroupOf(fh), -1: none; with sdso_shim::ImmaturePoints it is the
//                           frame's slot), the calibration and PRE_camToWorld; sets needRefresh (:85-165).  The points themselves stay
//                           in the map: a refresh reads the lists as they are then, which is what the reference shows too, since every
//                           publishKeyframes calls setFromKF first.
//   refreshPC(...)          the reference's needRefresh logic and return values (:176-200, :297-302, :322): false when nothing had to be
//                           done or the keyframe has no point, true after a rebuild — with no vertex the buffers stay as they were.
//   vertices() / colors() / numGLBufferGoodPoints stand for the two GL buffers: 3 floats and 3 bytes per vertex, camera frame (the
//                           reference's buffer; camToWorld is the member the caller puts into the GL matrix).  vertices_dev / colors_dev of
//                           the latest refresh of ANY display: sdso_map_cloud_dev.
//   refreshPC(displays, ..) the many-frames form: one sdso_map_cloud per 8 displays that need a refresh — a whole publishKeyframes call.
// Deviations (sdso_abi.h): no z jitter, and sparsity != 1 throws Error — both draw rand() in the reference.
template <class FrameHessianT, class CalibHessianT>
class KeyFrameDisplay {
 public:
  using SE3T = typename std::decay<decltype(std::declval<FrameHessianT>().PRE_camToWorld)>::type;
  KeyFrameDisplay(Device& dev, std::function<int(const FrameHessianT*)> immGroupOf = nullptr) : dev_(dev), imm_group_of_(std::move(immGroupOf)) {}
  int id = 0;                                                  // KeyFrameDisplay.h:91-93
  bool active = true;
  SE3T camToWorld;
  int numGLBufferGoodPoints = 0;                               // :118
  bool bufferValid = false;                                    // :116

  void setFromKF(FrameHessianT* fh, CalibHessianT* HCalib) {
    id = fh->shell->id;                                        // setFromF (:70-82)
    fx = HCalib->fxl(); fy = HCalib->fyl(); cx = HCalib->cxl(); cy = HCalib->cyl();
    frameID_ = fh->frameID;
    imm_group_ = imm_group_of_ ? imm_group_of_(fh) : -1;
    camToWorld = fh->PRE_camToWorld;                           // :163
    needRefresh = true;                                        // :164
    set_ = true;
  }
  bool refreshPC(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    std::vector<KeyFrameDisplay*> one{this};
    return refreshPC(one, canRefresh, scaledTH, absTH, mode, minBS, sparsity)[0];
  }
  static std::vector<bool> refreshPC(const std::vector<KeyFrameDisplay*>& displays, bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    if (sparsity != 1) throw Error("KeyFrameDisplay::refreshPC: sparsity != 1 draws rand() in the reference and is not built");
    std::vector<bool> ret(displays.size(), false);
    std::vector<size_t> todo;
    size_t at = 0;
    try {
    for (size_t i = 0; i < displays.size(); i++)
      if (displays[i]->begin_(canRefresh, scaledTH, absTH, mode, minBS, sparsity)) todo.push_back(i);
    for (; at < todo.size(); at += 8) {
      const int n = (int)std::min<size_t>(8, todo.size() - at);
      KeyFrameDisplay& d0 = *displays[todo[at]];
      int fid[8], imm[8], first[9];
      long bound = 0;
      for (int k = 0; k < n; k++) {
        KeyFrameDisplay& d = *displays[todo[at + k]];
        if (&d.dev_ != &d0.dev_ || d.fx != d0.fx || d.fy != d0.fy || d.cx != d0.cx || d.cy != d0.cy) throw Error("KeyFrameDisplay::refreshPC: the displays of one call share the device and the calibration");
        fid[k] = d.frameID_; imm[k] = d.imm_group_; bound += d.numSparsePoints_;
      }
      std::vector<float> xyz((size_t)bound * 8 * 3);
      std::vector<uint8_t> rgb((size_t)bound * 8 * 3);
      sdso_map_cloud_t Q;
      Q.n_frames = n; Q.frameID = fid; Q.imm_host_id = imm;
      Q.fx = d0.fx; Q.fy = d0.fy; Q.cx = d0.cx; Q.cy = d0.cy;
      Q.scaledTH = scaledTH; Q.absTH = absTH; Q.minBS = minBS; Q.mode = mode;
      Q.camToWorld = nullptr; Q.cap = (int)(bound * 8);
      d0.dev_.check(sdso_map_cloud(d0.dev_.ctx(), &Q, xyz.data(), rgb.data(), first, nullptr), "sdso_map_cloud");
      for (int k = 0; k < n; k++) {
        KeyFrameDisplay& d = *displays[todo[at + k]];
        ret[todo[at + k]] = true;
        const int nv = first[k + 1] - first[k];
        if (nv == 0) continue;                                 // :297-302: the buffers stay as they were
        d.numGLBufferGoodPoints = nv;                          // :304
        d.vertices_.assign(xyz.begin() + (size_t)first[k] * 3, xyz.begin() + (size_t)first[k + 1] * 3);
        d.colors_.assign(rgb.begin() + (size_t)first[k] * 3, rgb.begin() + (size_t)first[k + 1] * 3);
        d.bufferValid = true;                                  // :317
      }
    }
    } catch (...) {                                            // begin_() cleared needRefresh on displays whose buffers were not rebuilt
      for (size_t k = at; k < todo.size(); k++) displays[todo[k]]->needRefresh = true;
      throw;
    }
    return ret;
  }
  const std::vector<float>& vertices() const { return vertices_; }      // numGLBufferGoodPoints * 3
  const std::vector<uint8_t>& colors() const { return colors_; }

 private:
  // :176-200 up to "make data": true when the points have to be rebuilt
  bool begin_(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    if (!set_) throw Error("KeyFrameDisplay::refreshPC: setFromKF first");
    if (canRefresh)
      needRefresh = needRefresh || my_scaledTH != scaledTH || my_absTH != absTH || my_displayMode != mode || my_minRelBS != minBS || my_sparsifyFactor != sparsity;
    if (!needRefresh) return false;
    int c[3] = {0, 0, 0}, ni = 0;                              // (asked first: a refusal leaves needRefresh set)
    dev_.check(sdso_map_counts(dev_.ctx(), frameID_, c), "sdso_map_counts");
    if (imm_group_ >= 0) dev_.check(sdso_imm_count(dev_.ctx(), imm_group_, &ni), "sdso_imm_count");
    needRefresh = false;
    my_scaledTH = scaledTH; my_absTH = absTH; my_displayMode = mode; my_minRelBS = minBS; my_sparsifyFactor = sparsity;
    numSparsePoints_ = ni + c[0] + c[1] + c[2];                // :90-93
    return numSparsePoints_ != 0;                              // :199-200
  }
  Device& dev_;
  std::function<int(const FrameHessianT*)> imm_group_of_;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  bool needRefresh = true, set_ = false;                       // :57-67
  float my_scaledTH = 1e10f, my_absTH = 1e10f, my_minRelBS = 0;
  int my_displayMode = 1, my_sparsifyFactor = 1;
  int frameID_ = -1, imm_group_ = -1, numSparsePoints_ = 0;
  std::vector<float> vertices_;
  std::vector<uint8_t> colors_;
};

}  // namespace sdso_shim
