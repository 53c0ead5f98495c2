#pragma once
#include "device.h"
#include "marshal.h"
#include "selector.h"
namespace sdso_shim {
// ImmaturePointStatus ImmaturePoint::traceStereo(FrameHessian* frame, Mat33f K, bool mode_right) for a whole
// vector of points (the callers loop over all immature points: FullSystem.cpp:581-613, :667-725).
template <class ImmaturePointT, class Mat33fT>
inline void traceStereoAll(Device& dev, std::vector<ImmaturePointT*>& pts, int frame_slot, const Mat33fT& K, float baseline, bool mode_right,
                           std::vector<uint8_t>& status_out) {
  const int n = (int)pts.size();
  detail::TraceCols C(n);
  C.gather(pts, &ImmaturePointT::u_stereo, &ImmaturePointT::v_stereo, &ImmaturePointT::idepth_min_stereo, &ImmaturePointT::idepth_max_stereo);
  std::vector<float> imin(n), ids(n);
  for (int i = 0; i < n; i++) { imin[i] = pts[i]->idepth_min; ids[i] = pts[i]->idepth_stereo; }
  sdso_trace_points_t P = C.abi(imin.data(), ids.data());
  const float K4[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
  status_out.assign(n, 0);
  dev.check(sdso_trace_stereo_batch(dev.ctx(), frame_slot, K4, baseline, mode_right ? 1 : 0, &P, status_out.data()), "sdso_trace_stereo_batch");
  for (int i = 0; i < n; i++) { C.scatterTraced(i, pts[i], &ImmaturePointT::idepth_min_stereo, &ImmaturePointT::idepth_max_stereo); pts[i]->idepth_stereo = ids[i]; }
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
// ImmaturePoint::traceOn for all immature points of all host keyframes in the newest frame (FullSystem::traceNewCoarseKey / NonKey,
// FullSystem.cpp:632-790).  geom[h] = {KRKi, Kt, aff} of host h as computed at :654-665; host_of[i] selects it.
template <class ImmaturePointT>
inline void traceOnAll(Device& dev, std::vector<ImmaturePointT*>& pts, const std::vector<int>& host_of, const std::vector<sdso_trace_geom_t>& geom,
                       int frame_slot, std::vector<uint8_t>& status_out) {
  const int n = (int)pts.size();
  detail::TraceCols C(n);
  C.gather(pts, &ImmaturePointT::u, &ImmaturePointT::v, &ImmaturePointT::idepth_min, &ImmaturePointT::idepth_max);
  sdso_trace_points_t P = C.abi();
  status_out.assign(n, 0);
  dev.check(sdso_trace_on_batch(dev.ctx(), frame_slot, (int)geom.size(), geom.data(), host_of.data(), &P, status_out.data()), "sdso_trace_on_batch");
  for (int i = 0; i < n; i++) C.scatterTraced(i, pts[i], &ImmaturePointT::idepth_min, &ImmaturePointT::idepth_max);
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
namespace detail {
// a new ImmaturePoint object whose members the caller fills in: the stand-in types are default-constructible; the reference's class
// only has its two pixel constructors (ImmaturePoint.h:85-86), so the int one is used, which reads host->dI on the host and whose
// results are then overwritten
template <class P, class FrameHessianT, class CalibHessianT>
inline P* newImmaturePoint(std::true_type, float, float, FrameHessianT*, float, CalibHessianT*) { return new P(); }
template <class P, class FrameHessianT, class CalibHessianT>
inline P* newImmaturePoint(std::false_type, float u, float v, FrameHessianT* host, float type, CalibHessianT* HCalib) { return new P((int)u, (int)v, host, type, HCalib); }
}  // namespace detail
// ---- the device-resident immature points
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
template <class FrameHessianT, class CalibHessianT, class Mat33fT> class ImmaturePoints {
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
    float Kf[9], Kif[9], Rf[9], Rif[9], KR[9];
    detail::toFloat9(K, Kf); detail::toFloat9(Ki, Kif); detail::toFloat9(R, Rf); detail::toFloat9(Ri, Rif);
    sdso_imm_geom_t g;
    g.host_id = slot_of_(host);
    for (int i = 0; i < 3; i++) g.t[i] = (float)t[i];
    detail::mul33(Kf, Rf, KR); detail::mul33(KR, Kif, g.KRKi);
    detail::mul33(Kf, Rif, g.KRi);
    detail::mul31(Kf, g.t, g.Kt);
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
    detail::TraceCols C(n);
    std::vector<float> ty(n);
    sdso_trace_points_t P = C.abi();
    if (n) dev_.check(sdso_imm_get(dev_.ctx(), slot_of_(host), &P, ty.data()), "sdso_imm_get");
    for (ImmaturePointT* p : host->immaturePoints) delete p;
    host->immaturePoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
      ImmaturePointT* p = detail::newImmaturePoint<ImmaturePointT>(std::is_default_constructible<ImmaturePointT>(), C.u[i], C.v[i], host, ty[i], &Hcalib_);
      p->host = host; p->idxInImmaturePoints = i; p->my_type = ty[i];
      C.scatterTraced(i, p, &ImmaturePointT::idepth_min, &ImmaturePointT::idepth_max); C.scatterFixed(i, p);
      host->immaturePoints[i] = p;
    }
  }
  // The loop of FullSystem::stereoMatch (FullSystem.cpp:579-613) after makeNewTraces(fh, fh_right, 0): every point of fh traced into
  // fh_right and back, the accept rule of :601 with the reference's depth < 70, and for every accepted point idepth_stereo, idepth_min,
  // idepth_max at (float*)(idepthMap.data + int(v) * idepthMap.step) + (int)u * 3.  No other pixel is touched, as in the reference; returns
  // `counter`.  MatT: the reference's cv::Mat (CV_32FC3), or anything with `unsigned char* data` and `size_t step`.  The traces and the
  // rule run on the device (sdso_imm_stereo_match); 13 bytes per point come back, and u, v (8 more) for the pixel.  fh->immaturePoints is
  // not touched and the group stays in the set: release(fh) goes where the reference deletes fh.
  template <class MatT> int stereoMatch(FrameHessianT* fh, FrameHessianT* fh_right, MatT& idepthMap) {
    const int n = count(fh);
    std::vector<uint8_t> accepted(n);
    std::vector<float> idepth((size_t)n * 3), us(n), vs(n);
    sdso_imm_match_out_t O{accepted.data(), idepth.data(), nullptr, nullptr, nullptr};
    float K4[4]; detail::calibK4(Hcalib_, K4);                   // K of :569-573
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
    detail::TraceCols C(n);
    C.gather(host->immaturePoints, &ImmaturePointT::u, &ImmaturePointT::v, &ImmaturePointT::idepth_min, &ImmaturePointT::idepth_max);
    std::vector<float> ty(n);
    for (int i = 0; i < n; i++) ty[i] = host->immaturePoints[i]->my_type;
    const sdso_trace_points_t P = C.abi();
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
                          {}, minObs, currentMinActDist, setting_minTraceQuality};
    detail::calibK4(Hcalib_, A.K);
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
    detail::pinholeK(K, Hcalib_.fxl(), Hcalib_.fyl(), Hcalib_.cxl(), Hcalib_.cyl());
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
    detail::toFloat9(Ki, Ki9);
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
}  // namespace sdso_shim
