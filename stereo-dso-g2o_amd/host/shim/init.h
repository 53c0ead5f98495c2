#pragma once
#include <cstdlib>
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
// class CoarseInitializer (FullSystem/CoarseInitializer.h), the part the stereo fork runs: setFirstStereo (CoarseInitializer.cpp:838-1034,
// called at FullSystem.cpp:1092-1093) and what FullSystem::initializeFromInitializer reads of it (FullSystem.cpp:1487-1597: firstFrame,
// firstRightFrame, thisToNext, numPoints[0], points[0]), on the initialiser state of the Device's ctx (sdso_init_*).  Levels >= 1, makeNN,
// dGrads, setFirst, trackFrame and calcResAndGS are not mirrored: their only reader is the monocular trackFrame, which the fork never calls.
// (ww, hh) is the reference's constructor pair; slot_of(frame) is the frame's pyramid slot on the device, the first frame's with levels
// 0..2 (the selector).  SE3T is the reference's Sophus::SE3d.
template <class FrameHessianT, class CalibHessianT, class SE3T> class CoarseInitializer {
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
    detail::calibK4(*HCalib, K_);             // :853-857
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
}  // namespace sdso_shim
