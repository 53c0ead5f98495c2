// float FullSystem::optimize(int mnumOptIts) as the fork compiles it (FullSystem/FullSystemOptimize.cpp:402-868): the body between STEP1
// (activeResiduals collected, :437-453) and the applyRes that follows the write-back (:729-733) becomes
//     return sdso_shim::optimizeForkLive(dev, frameHessians, activeResiduals, Hcalib, slot_of, mnumOptIts, wG[0], hG[0]);
// It flattens the graph of :455-542 — one pose + one photometric vertex per host frame, one idepth vertex per residual, the camera —
// makes ONE sdso_g2o_lba_optimize call and performs the write-back of :682-727 in activeResiduals order, so that the last residual of a
// point wins setIdepth, as in the reference (an INACTIVE last residual hands the point its old idepth back: its vertex never moved).
// g2o's graph plumbing is not rebuilt; what g2o decides is a restatement (include/sdso_abi.h at the call).
//   written   Hcalib.value / value_scaled / value_scaledf / value_scaledi / value_minus_value_zero                          :682-696
//             per host named by a residual: PRE_camToWorld, PRE_worldToCam (its inverse), state[6..7], state_scaled[6..7]     :703-720
//             per residual: centerProjectedTo, point->setIdepth / setIdepthZero, efResidual->point->HdiF                     :722-726
//             per residual, for the applyRes that follows (:764): state_NewState, state_NewEnergy, state_NewEnergyWithOutlier
//   idepth_hessian : linearizeOplus writes r->point->idepth_hessian (dso_g2o_edge.cpp:270) unless it returns early; here the point takes
//             the value of its residuals in activeResiduals order, where the last linearisation produced one (non-zero), before :726 reads it
//   mnumOptIts: as given; the 10 / 7 / 3 rule of :406-418 is the caller's
//   returns   the rmse of :867
//
// Three routes over ONE flatten and ONE write-back (ForkLiveCall below):
//   optimizeForkLive                  sdso_g2o_lba_optimize: the loop's controller on the host, a launch and a wait per evaluation
//   optimizeForkLiveResident          sdso_g2o_lba_optimize_resident: the controller resident on the device, one wait at the end
//   optimizeForkLiveBegin / ..End     the same, split: Begin flattens and enqueues and returns at once, End waits and writes back; the caller
//                                     puts host work between them.  Between Begin and End the window's frames keep their slots, nothing
//                                     the write-back touches is read or written by that host work, and activeResiduals / Hcalib given to
//                                     End are those given to Begin.  One job per Device.
//
// This header sits beside sdso_shim.h, not under shim/: the parts there are the DSO-native call surface, and their set is pinned
// (tests/test_host_shim.py::test_shim_parts_are_all_there); the fork-live layer is included by the umbrella all the same.
#pragma once
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "shim/device.h"
#include "shim/marshal.h"
namespace sdso_shim {
// The graph of :455-542 as the arrays of one call, and the write-back of :682-727 from what the call left in them.
struct ForkLiveCall {
  int nf = 0, nr = 0;
  std::vector<int> slot, host, target;
  std::vector<sdso_se3_t> Ttw, Twh;
  std::vector<sdso_aff_t> target_aff, host_aff;
  std::vector<float> exposure, eTH, u, v, color, weights;
  std::vector<double> b0, idepth;
  std::vector<uint8_t> state, level, active;
  std::vector<float> energy, cpt, ih;
  sdso_g2o_lba_window_t W;
  sdso_g2o_lba_state_t S;
  sdso_g2o_lba_opt_t P;
  sdso_g2o_lba_result_t out;
  ForkLiveCall() {}
  ForkLiveCall(const ForkLiveCall&) = delete;             // (W, S and out point into the vectors: moved, never copied)
  ForkLiveCall& operator=(const ForkLiveCall&) = delete;
  ForkLiveCall(ForkLiveCall&&) = default;
  ForkLiveCall& operator=(ForkLiveCall&&) = default;

  template <class FrameHessianT, class PointFrameResidualT, class CalibHessianT, class SlotOf>
  void flatten(std::vector<FrameHessianT*>& frameHessians, std::vector<PointFrameResidualT*>& activeResiduals, CalibHessianT& Hcalib, SlotOf slot_of,
               int mnumOptIts, int w, int h, const char* who) {
    nf = (int)frameHessians.size(); nr = (int)activeResiduals.size();
    if (nf < 1 || nf > 8) throw Error(std::string(who) + ": 1..8 frames");
    slot.resize(nf); host.resize(nr); target.resize(nr);
    Ttw.resize(nf); Twh.resize(nf); target_aff.resize(nf); host_aff.resize(nf);
    exposure.resize(nf); eTH.resize(nf); u.resize(nr); v.resize(nr); color.resize((size_t)nr * 8); weights.resize((size_t)nr * 8);
    b0.resize(nf); idepth.resize(nr);
    for (int f = 0; f < nf; f++) {
      FrameHessianT* fh = frameHessians[f];
      slot[f] = slot_of(fh);
      Ttw[f] = toAbi(fh->PRE_worldToCam);                      // dso_g2o_edge.cpp:23
      Twh[f] = toAbi(fh->PRE_camToWorld);                      // :485
      const auto a = fh->aff_g2l();                            // :490, dso_g2o_edge.cpp:87
      target_aff[f] = sdso_aff_t{a.a, a.b};
      host_aff[f] = sdso_aff_t{a.a, a.b};
      b0[f] = a.b;                                             // SetB, :535-536
      exposure[f] = fh->ab_exposure; eTH[f] = fh->frameEnergyTH;
    }
    for (int r = 0; r < nr; r++) {
      const PointFrameResidualT* pfr = activeResiduals[r];
      host[r] = pfr->host->idx; target[r] = pfr->target->idx;
      u[r] = pfr->point->u; v[r] = pfr->point->v;
      idepth[r] = pfr->point->idepth;                          // :507
      for (int k = 0; k < 8; k++) { color[(size_t)r * 8 + k] = pfr->point->color[k]; weights[(size_t)r * 8 + k] = pfr->point->weights[k]; }
    }
    W = sdso_g2o_lba_window_t{nf, nr, w, h, slot.data(), Ttw.data(), target_aff.data(), exposure.data(), b0.data(), eTH.data(),
                              host.data(), target.data(), u.data(), v.data(), color.data(), weights.data()};
    S = sdso_g2o_lba_state_t{Twh.data(), host_aff.data(), {Hcalib.fxl(), Hcalib.fyl(), Hcalib.cxl(), Hcalib.cyl()}, idepth.data()};   // :458
    P = sdso_g2o_lba_opt_t{mnumOptIts, 0.1, 1e-3, 10};         // :426, :432, g2o's maxTrialsAfterFailure
    state.assign(nr, 0); level.assign(nr, 0); active.assign(nr, 0);
    energy.assign((size_t)nr * 2, 0.f); cpt.assign((size_t)nr * 3, 0.f); ih.assign(nr, 0.f);
    out = sdso_g2o_lba_result_t{};
    out.state = state.data(); out.energy = energy.data(); out.centerProjectedTo = cpt.data(); out.edge_level = level.data();
    out.idepth_hessian = ih.data(); out.active = active.data();
  }

  // returns the rmse of :867
  template <class PointFrameResidualT, class CalibHessianT>
  float writeBack(std::vector<PointFrameResidualT*>& activeResiduals, CalibHessianT& Hcalib) {
    using SE3T = typename std::decay<decltype(activeResiduals[0]->host->PRE_camToWorld)>::type;
    using Mat33T = typename std::decay<decltype(std::declval<SE3T>().rotationMatrix())>::type;
    using Vec3T = typename std::decay<decltype(std::declval<SE3T>().translation())>::type;
    if ((int)activeResiduals.size() != nr) throw Error("optimizeForkLive: activeResiduals changed between flatten and write-back");
    // ---- :682-696
    for (int i = 0; i < 4; i++) {
      Hcalib.value[i] = S.cam[i];
      Hcalib.value_scaled[i] = 1 * Hcalib.value[i];
      Hcalib.value_scaledf[i] = (float)Hcalib.value_scaled[i];
    }
    Hcalib.value_scaledi[0] = 1.0f / Hcalib.value_scaledf[0];
    Hcalib.value_scaledi[1] = 1.0f / Hcalib.value_scaledf[1];
    Hcalib.value_scaledi[2] = -Hcalib.value_scaledf[2] / Hcalib.value_scaledf[0];
    Hcalib.value_scaledi[3] = -Hcalib.value_scaledf[3] / Hcalib.value_scaledf[1];
    for (int i = 0; i < 4; i++) Hcalib.value_minus_value_zero[i] = Hcalib.value[i] - Hcalib.value_zero[i];
    // ---- :699-727
    bool vtxused2[8] = {false};
    for (int r = 0; r < nr; r++) {
      PointFrameResidualT* pfr = activeResiduals[r];
      const int hi = pfr->host->idx;
      if (!vtxused2[hi]) {
        vtxused2[hi] = true;
        pfr->host->PRE_camToWorld = fromAbi<SE3T, Mat33T, Vec3T>(Twh[hi]);
        pfr->host->PRE_worldToCam = pfr->host->PRE_camToWorld.inverse();
        pfr->host->state[6] = host_aff[hi].a;
        pfr->host->state[7] = host_aff[hi].b;
        pfr->host->state_scaled[6] = 1 * pfr->host->state[6];
        pfr->host->state_scaled[7] = 1 * pfr->host->state[7];
      }
      for (int k = 0; k < 3; k++) pfr->centerProjectedTo[k] = cpt[(size_t)r * 3 + k];
      pfr->point->setIdepth(idepth[r]);
      pfr->point->setIdepthZero(idepth[r]);
      if (ih[r] != 0) pfr->point->idepth_hessian = ih[r];
      pfr->efResidual->point->HdiF = 1.0 / pfr->point->idepth_hessian;
      pfr->state_NewState = static_cast<typename std::decay<decltype(pfr->state_NewState)>::type>(state[r]);
      pfr->state_NewEnergy = energy[(size_t)r * 2];
      pfr->state_NewEnergyWithOutlier = energy[(size_t)r * 2 + 1];
    }
    return out.rmse;
  }
};

template <class FrameHessianT, class PointFrameResidualT, class CalibHessianT, class SlotOf>
inline float optimizeForkLive(Device& dev, std::vector<FrameHessianT*>& frameHessians, std::vector<PointFrameResidualT*>& activeResiduals,
                              CalibHessianT& Hcalib, SlotOf slot_of, int mnumOptIts, int w, int h) {
  ForkLiveCall C;
  C.flatten(frameHessians, activeResiduals, Hcalib, slot_of, mnumOptIts, w, h, "optimizeForkLive");
  dev.check(sdso_g2o_lba_optimize(dev.ctx(), &C.W, &C.P, &C.S, &C.out), "sdso_g2o_lba_optimize");
  return C.writeBack(activeResiduals, Hcalib);
}

template <class FrameHessianT, class PointFrameResidualT, class CalibHessianT, class SlotOf>
inline float optimizeForkLiveResident(Device& dev, std::vector<FrameHessianT*>& frameHessians, std::vector<PointFrameResidualT*>& activeResiduals,
                                      CalibHessianT& Hcalib, SlotOf slot_of, int mnumOptIts, int w, int h) {
  ForkLiveCall C;
  C.flatten(frameHessians, activeResiduals, Hcalib, slot_of, mnumOptIts, w, h, "optimizeForkLiveResident");
  dev.check(sdso_g2o_lba_optimize_resident(dev.ctx(), &C.W, &C.P, &C.S, &C.out), "sdso_g2o_lba_optimize_resident");
  return C.writeBack(activeResiduals, Hcalib);
}

// the call between Begin and End: the library has copied every input, this keeps where the results go
typedef ForkLiveCall ForkLiveJob;
template <class FrameHessianT, class PointFrameResidualT, class CalibHessianT, class SlotOf>
inline ForkLiveJob optimizeForkLiveBegin(Device& dev, std::vector<FrameHessianT*>& frameHessians, std::vector<PointFrameResidualT*>& activeResiduals,
                                         CalibHessianT& Hcalib, SlotOf slot_of, int mnumOptIts, int w, int h) {
  ForkLiveJob C;
  C.flatten(frameHessians, activeResiduals, Hcalib, slot_of, mnumOptIts, w, h, "optimizeForkLiveBegin");
  dev.check(sdso_g2o_lba_optimize_enqueue(dev.ctx(), &C.W, &C.P, &C.S), "sdso_g2o_lba_optimize_enqueue");
  return C;
}
template <class PointFrameResidualT, class CalibHessianT>
inline float optimizeForkLiveEnd(Device& dev, ForkLiveJob& job, std::vector<PointFrameResidualT*>& activeResiduals, CalibHessianT& Hcalib) {
  dev.check(sdso_g2o_lba_optimize_fetch(dev.ctx(), &job.S, &job.out), "sdso_g2o_lba_optimize_fetch");
  return job.writeBack(activeResiduals, Hcalib);
}
}  // namespace sdso_shim
