#pragma once
#include "device.h"
namespace sdso_shim {
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
template <class BA> class AccumulatedTopHessianSSE {
 public:
  explicit AccumulatedTopHessianSSE(BA& ba) : ba_(ba) { for (int i = 0; i < 6; i++) { nframes[i] = 0; nres[i] = 0; } }
  int nframes[6];   // NUM_THREADS (util/NumType.h:38)
  int nres[6];
  template <class StatsT = void> void setZero(int nFrames, int /*min*/ = 0, int /*max*/ = 1, StatsT* /*stats*/ = 0, int tid = 0) {
    nframes[tid] = nFrames; nres[tid] = 0; mode_ = -1; flagged_.clear();
  }
  template <int mode, class EFPointT, class EFT> void addPoint(EFPointT* p, EFT const* /*ef*/, int /*tid*/ = 0) {
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
template <class BA> class AccumulatedSCHessianSSE {
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
  template <class MatXX, class VecX, class EFT> void stitchDouble(MatXX& H, VecX& b, EFT const* /*EF*/, int /*tid*/ = 0) { stitch_(H, b); }
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
}  // namespace sdso_shim
