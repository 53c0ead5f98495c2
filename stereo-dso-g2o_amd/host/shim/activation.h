#pragma once
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
// class CoarseDistanceMap (FullSystem/CoarseTracker.h:165-197) with the members its caller (FullSystem::activatePointsMT,
// FullSystem.cpp:823-902) touches: makeK(CalibHessian*), makeDistanceMap(frameHessians, frame), addIntoDistFinal(u, v),
// fwdWarpedIDDistFinal, K[], Ki[].  The map itself lives on the device (one per Device); fwdWarpedIDDistFinal is a host copy that
// distFinal() refreshes on demand.  Mat33fT / Vec3fT are the reference's Eigen float types (element access (i, j) / [i]; an
// `inverse()` member is used where the type has one).  The float products K[1] * R * Ki[0] and K[1] * t are formed here, row times
// column summed left to right (detail::mul33 / mul31).
template <class Mat33fT> class CoarseDistanceMap {
 public:
  CoarseDistanceMap(Device& dev, int ww, int hh) : dev_(dev), buf_((size_t)(ww / 2) * (hh / 2), 1000.f) {
    fwdWarpedIDDistFinal = buf_.data();
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) w[l] = h[l] = 0;
  }
  // makeK(CalibHessian*) — CoarseTracker.cpp:1374-1402 (pyrLevelsUsed and wG[0] / hG[0] are globals in the reference)
  template <class CalibHessianT> void makeK(CalibHessianT* HCalib, int pyrLevelsUsed, int wG0, int hG0) {
    detail::levelIntrinsics(HCalib, pyrLevelsUsed, wG0, hG0, w, h, fx, fy, cx, cy);
    for (int level = 0; level < pyrLevelsUsed; ++level) {
      detail::pinholeK(K[level], fx[level], fy[level], cx[level], cy[level]);
      Ki[level] = detail::inverse33(K[level], 0);
      fxi[level] = Ki[level](0, 0); fyi[level] = Ki[level](1, 1); cxi[level] = Ki[level](0, 2); cyi[level] = Ki[level](1, 2);
    }
  }
  // KRKi = K[1] * fhToNew.rotationMatrix().cast<float>() * Ki[0], Kt = K[1] * fhToNew.translation().cast<float>() with
  // fhToNew = frame->PRE_worldToCam * fh->PRE_camToWorld (CoarseTracker.cpp:1232-1236, FullSystem.cpp:840-842)
  template <class FrameHessianT> sdso_distmap_geom_t geomOf(const FrameHessianT* fh, const FrameHessianT* frame) const {
    const auto fhToNew = frame->PRE_worldToCam * fh->PRE_camToWorld;
    const auto R = fhToNew.rotationMatrix();
    const auto t = fhToNew.translation();
    float K1[9], Ki0[9], Rf[9], KR[9];
    detail::toFloat9(K[1], K1); detail::toFloat9(Ki[0], Ki0); detail::toFloat9(R, Rf);
    const float tf[3] = {(float)t[0], (float)t[1], (float)t[2]};
    sdso_distmap_geom_t g;
    detail::mul33(K1, Rf, KR); detail::mul33(KR, Ki0, g.KRKi);
    detail::mul31(K1, tf, g.Kt);
    return g;
  }
  // makeDistanceMap(std::vector<FrameHessian*> frameHessians, FrameHessian* frame) — CoarseTracker.cpp:1216-1255
  template <class FrameHessianT> void makeDistanceMap(std::vector<FrameHessianT*> frameHessians, FrameHessianT* frame) {
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
}  // namespace sdso_shim
