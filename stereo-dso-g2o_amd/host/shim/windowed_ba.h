#pragma once
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
namespace detail {   // the bodies of WindowedBA that touch only the caller's pointer graph or plain buffers
// EFPointStatus (EnergyFunctionalStructs.h:97): PS_GOOD = 0, PS_MARGINALIZE = 1, PS_DROP = 2
template <class EFPointT> inline void setStateFlag(EFPointT* p, int v) { p->stateFlag = static_cast<std::decay_t<decltype(p->stateFlag)>>(v); }
template <class List> inline void swapOut(List& list, size_t i) { list[i] = list.back(); list.pop_back(); }
template <class FrameHessianT, class PointHessianT> inline void dropOut(FrameHessianT* host, PointHessianT* ph) { host->pointHessiansOut.push_back(ph); setStateFlag(ph->efPoint, 2); }
template <class PH, class PFR> inline auto lastResidualOf(PH* ph, const PFR* pfr) -> decltype(&ph->lastResiduals[0]) {   // the entry that names pfr, or null
  return ph->lastResiduals[0].first == pfr ? &ph->lastResiduals[0] : ph->lastResiduals[1].first == pfr ? &ph->lastResiduals[1] : nullptr;
}
// FullSystem::removeOutliers' loop (FullSystemOptimize.cpp:1066-1081) with `ph->residuals.size() == 0` (:1073) decided by decision(efPoint)
template <class FrameHessians, class Decision> inline void dropPointsWithoutResiduals(FrameHessians& frameHessians, Decision decision, int& numPointsDropped) {
  for (auto* fh : frameHessians)
    for (unsigned int i = 0; i < fh->pointHessians.size(); i++) {
      auto* ph = fh->pointHessians[i];
      if (ph == 0 || decision(ph->efPoint) != SDSO_PT_DROP_NO_RESIDUAL) continue;
      dropOut(fh, ph);
      swapOut(fh->pointHessians, i);
      i--;
      numPointsDropped++;
    }
}
// FullSystem::flagPointsForRemoval's loop (FullSystem.cpp:983-1054) with the tests on the point replaced by decision(efPoint)
template <class FrameHessians, class Decision>
inline void flagPointsInLists(FrameHessians& frameHessians, Decision decision, int& flag_oob, int& flag_in, int& flag_inin, int& flag_nores) {
  for (auto* host : frameHessians) {
    for (unsigned int i = 0; i < host->pointHessians.size(); i++) {
      auto* ph = host->pointHessians[i];
      if (ph == 0) continue;
      const int d = decision(ph->efPoint);
      if (d == SDSO_PT_KEEP) continue;
      if (d == SDSO_PT_DROP_NEGATIVE || d == SDSO_PT_DROP_NO_RESIDUAL) {                   // FullSystem.cpp:997-1002
        dropOut(host, ph);
        flag_nores++;
      } else {                                                                             // :1004-1041: isOOB or the host leaves
        flag_oob++;
        if (d == SDSO_PT_MARGINALIZE || d == SDSO_PT_DROP_WEAK) flag_in++;                 // isInlierNew
        if (d == SDSO_PT_MARGINALIZE) {
          flag_inin++;
          setStateFlag(ph->efPoint, 1);
          host->pointHessiansMarginalized.push_back(ph);
        } else dropOut(host, ph);
      }
      host->pointHessians[i] = 0;
    }
    for (int i = 0; i < (int)host->pointHessians.size(); i++)                              // :1044-1051
      if (host->pointHessians[i] == 0) { swapOut(host->pointHessians, i); i--; }
  }
}
// optimize()'s write-back (FullSystemOptimize.cpp:871-1041); points are EFPoint*, residuals EFResidual*, both in window order
template <class EnergyFunctionalT, class CalibHessianT, class Points, class Residuals>
inline void writeBackPostState(EnergyFunctionalT* ef, CalibHessianT* HCalib, int nf, const Points& points, const Residuals& residuals, const sdso_ba_post_state_t& P, bool stats) {
  auto v = HCalib->value_zero;                           // a VecC to fill
  for (int i = 0; i < 4; i++) v[i] = P.calib_value[i];
  HCalib->setValue(v);
  for (int i = 0; i < 4; i++) HCalib->step[i] = P.calib_step[i];
  for (int f = 0; f < nf; f++) {
    auto* fh = ef->frames[f]->data;
    auto s = fh->get_state();                            // a Vec10 to fill
    for (int i = 0; i < 10; i++) s[i] = P.state[f * 10 + i];
    if (f == nf - 1) {
      // setEvalPT(PRE_worldToCam at the loop's final state, {0,..,0, a, b, 0, 0}) (:997-1003); the frame's own SE3 lends its types
      sdso_se3_t T;
      std::memcpy(T.R, &P.evalPT[f * 12], 72); std::memcpy(T.t, &P.evalPT[f * 12 + 9], 24);
      const auto& proto = fh->get_worldToCam_evalPT();
      fh->setEvalPT(fromAbi<std::decay_t<decltype(proto)>, std::decay_t<decltype(proto.rotationMatrix())>, std::decay_t<decltype(proto.translation())>>(T), s);
    } else fh->setState(s);
    for (int i = 0; i < 10; i++) fh->step[i] = P.frame_step[f * 10 + i];
    fh->frameEnergyTH = P.frameEnergyTH[f];
  }
  for (size_t p = 0; p < points.size(); p++) {
    auto* efp = points[p];
    auto* ph = efp->data;
    ph->setIdepth(P.idepth[p]); ph->setIdepthZero(P.idepth[p]);
    ph->step = P.step[p];
    if (stats) { ph->idepth_hessian = P.idepth_hessian[p]; ph->maxRelBaseline = P.maxRelBaseline[p]; ph->numGoodResiduals = P.numGoodResiduals[p]; }
    efp->HdiF = P.HdiF[p]; efp->bdSumF = P.bdSumF[p];
  }
  for (size_t i = 0; i < residuals.size(); i++) {          // the projections are written where P binds them
    auto* r = residuals[i];
    auto* pfr = r->data;
    if (r->isLinearized) continue;                       // not in activeResiduals (:880-889): optimize() never touches it
    using ResStateT = std::decay_t<decltype(pfr->state_state)>;
    pfr->state_state = static_cast<ResStateT>(P.state_state[i]);
    pfr->state_NewState = static_cast<ResStateT>(P.state_state[i]);
    pfr->state_energy = P.state_energy[i]; pfr->state_NewEnergy = P.state_energy[i];
    r->isActiveAndIsGoodNEW = P.isActiveAndIsGoodNEW[i] != 0;
    if (P.isActiveAndIsGoodNEW[i] && P.centerProjectedTo) {
      for (int k = 0; k < 3; k++) pfr->centerProjectedTo[k] = P.centerProjectedTo[i * 3 + k];
      for (int k = 0; k < 8; k++) { pfr->projectedTo[k][0] = P.projectedTo[i * 16 + 2 * k]; pfr->projectedTo[k][1] = P.projectedTo[i * 16 + 2 * k + 1]; }
    }
    if (auto* last = lastResidualOf(pfr->point, pfr)) last->second = pfr->state_state;   // :165-172
  }
}
// the toRemove sweep (:176-195) with deleteOut (FullSystem.h:62-71); dropped(i, pfr) runs between dropResidual and `delete pfr`
template <class EnergyFunctionalT, class Residuals, class Dropped>
inline int dropRemovedResiduals(EnergyFunctionalT* ef, Residuals& residuals, const uint8_t* toRemove, Dropped dropped) {
  int nResRemoved = 0;
  for (size_t i = 0; i < residuals.size(); i++) {
    if (!toRemove[i] || residuals[i]->isLinearized) continue;
    auto* pfr = residuals[i]->data;
    auto* ph = pfr->point;
    if (auto* last = lastResidualOf(ph, pfr)) last->first = 0;
    for (unsigned int k = 0; k < ph->residuals.size(); k++)
      if (ph->residuals[k] == pfr) {
        ef->dropResidual(pfr->efResidual);
        dropped((int)i, pfr);
        delete ph->residuals[k];
        swapOut(ph->residuals, k);
        nResRemoved++;
        break;
      }
  }
  return nResRemoved;
}
}  // namespace detail
// Flattens the reference's pointer graph (EnergyFunctional::frames -> EFFrame::points -> EFPoint::residualsAll,
// i.e. makeIDX order, EnergyFunctional.cpp:998-1018) into sdso_ba_window_t and drives the device window.
// slot_of(FrameHessian*) returns the pyramid slot the frame was uploaded to.
template <class EnergyFunctionalT, class CalibHessianT> class WindowedBA {
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
    F.bind(W);
    W.u = P.u.data(); W.v = P.v.data(); W.idepth = P.idepth.data(); W.idepth_zero = P.idepth_zero.data();
    W.color = P.color.data(); W.weights = P.weights.data(); W.host = P.host.data(); W.hasDepthPrior = P.prior.data();
    W.res_point = R.point.data(); W.res_target = R.target.data(); W.res_state = R.state.data();
    W.maxRelBaseline = P.maxRelBaseline.data(); W.numGoodResiduals = P.numGood.data(); W.res_isNew = R.isNew.data();
    const int n = dim_(nf);
    HM_.assign((size_t)n * n, 0); bM_.assign(n, 0);
    for (int i = 0; i < n; i++) { bM_[i] = ef->bM[i]; for (int j = 0; j < n; j++) HM_[(size_t)i * n + j] = ef->HM(i, j); }
    W.HM = HM_.data(); W.bM = bM_.data();
    W.solverMode = solverMode; W.affineOptModeA = affineOptModeA; W.affineOptModeB = affineOptModeB; W.forceAcceptStep = forceAcceptStep ? 1 : 0;
    dev_.check(sdso_ba_upload_window(dev_.ctx(), win_, &W), "sdso_ba_upload_window");
    nf_ = nf; resInM_seen_ = 0; ef_ = ef;
    reindex_();
    stateMoved_();
    frames_.assign(ef->frames.begin(), ef->frames.end());
    clearPending_();
    window_serial_++;
  }

  // Vec3 FullSystem::linearizeAll(false): returns lastEnergyP
  double linearizeAll() {
    double e = 0;
    dev_.check(sdso_ba_linearize(dev_.ctx(), win_, &e), "sdso_ba_linearize");
    stateMoved_();
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
  template <class PointFrameResidualT> double linearize(PointFrameResidualT* r, CalibHessianT* /*HCalib*/) {
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
  template <class PointFrameResidualT> void applyRes(PointFrameResidualT* r, bool copyJacobians) {
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
    lastX.assign(dim_(nf_), 0); frame_step.assign(nf_ * 8, 0);
    ensureAccumulated();
    dev_.check(sdso_ba_solve(dev_.ctx(), win_, iteration, lambda, lastX.data(), nullptr, nullptr, frame_step.data(), calib_step), "sdso_ba_solve");
  }
  // void EnergyFunctional::solveSystemF(int iteration, double lambda, CalibHessian* HCalib) — EnergyFunctional.h:74, EnergyFunctional.cpp:838-995
  // with resubstituteF_MT (:272-341) — verbatim: everything the reference's function leaves in its objects is written into them:
  //   ef->lastX, lastHS, lastbS (:909-910, :992); ef->resInA / resInL (:219, :241); HCalib->step = -x.head<CPARS>() (:279);
  //   every EFFrame::data->step.head<8>() = -x.segment<8>(CPARS + 8 idx), tail<2>() = 0 (:283-286);
  //   every PointHessian::step (:336-338), EFPoint::HdiF / bdSumF (AccumulatedSCHessian.cpp:58-65)
  void solveSystemF(int iteration, double lambda, CalibHessianT* HCalib) {
    const int n = dim_(nf_), np = (int)points_.size();
    std::vector<double> x(n), HS((size_t)n * n), bS(n), fstep(nf_ * 8);
    double cstep[4];
    ensureAccumulated();
    dev_.check(sdso_ba_solve(dev_.ctx(), win_, iteration, lambda, x.data(), HS.data(), bS.data(), fstep.data(), cstep), "sdso_ba_solve");
    writeLastSystem_(ef_, x.data(), HS.data(), bS.data(), n);
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
    delete[] ef_->adHost; delete[] ef_->adTarget; delete[] ef_->adHostF; delete[] ef_->adTargetF;   // (null where none were made yet)
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
    delete[] ef_->adHTdeltaF; ef_->adHTdeltaF = new M18f[nf * nf];
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
    marginalised_();
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
    const int nf = nf_, np = (int)points_.size(), nr = (int)residuals_.size(), n = dim_(nf_);
    sdso_ba_opt_result_t out;
    stateMoved_();
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
    detail::writeBackPostState(ef, HCalib, nf, points_, residuals_, P, writeBackPointStats);
    // (dropResidual deletes a residual: its slot in residuals_ is null until update() — or upload() — brings the device window in line)
    lastRemoved = detail::dropRemovedResiduals(ef, residuals_, P.toRemove, [this](int i, const void* pfr) {
      res_index_.erase(pfr); residuals_[i] = nullptr; pending_drop_res_.push_back(i);   // stage 1 of the next update(), in toRemove order
    });
    writeLastSystem_(ef, P.lastX, P.lastHS, P.lastbS, n);
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
  template <class FrameHessians> void removeOutliers(FrameHessians& frameHessians) {
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
    detail::dropPointsWithoutResiduals(frameHessians, [this](const void* efPoint) { return decisionOf_(efPoint, "removeOutliers"); }, numPointsDropped);
  }
  template <class FrameHessians> void flagPointsForRemoval(FrameHessians& frameHessians) {
    if (!flags_pending_) throw Error("flagPointsForRemoval: no decisions are pending: removeOutliers() makes them, once per optimize()");
    if (flags_serial_ != window_serial_) throw Error("flagPointsForRemoval: the device window was edited since removeOutliers() (update() / upload() come after it)");
    flag_oob = flag_in = flag_inin = flag_nores = 0;
    detail::flagPointsInLists(frameHessians, [this](const void* efPoint) { return decisionOf_(efPoint, "flagPointsForRemoval"); },
                              flag_oob, flag_in, flag_inin, flag_nores);
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
  template <class IsMarg> void marginalizePointsF(EnergyFunctionalT* ef, IsMarg is_marg) {
    requireNoPendingEdit_("marginalizePointsF");
    std::vector<uint8_t> flag(points_.size());
    for (size_t p = 0; p < points_.size(); p++) flag[p] = is_marg(points_[p]) ? 1 : 0;
    dev_.check(sdso_ba_marginalize_points(dev_.ctx(), win_, flag.data(), HM_.data(), bM_.data()), "sdso_ba_marginalize_points");
    marginalised_();
    detail::fill(ef->bM, bM_.data(), dim_(nf_)); detail::fill(ef->HM, HM_.data(), dim_(nf_), dim_(nf_));
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
  template <class EFPointT> void willRemovePoint(EFPointT* p) {
    const int i = point_index_.at(p);
    pending_rm_points_.push_back(i);
    forgetPoint_(i);
  }
  template <class IsDrop> void willDropPoints(IsDrop is_drop) {
    if (pending_drop_flags_.empty()) pending_drop_flags_.assign(points_.size(), 0);
    for (size_t i = 0; i < points_.size(); i++)
      if (points_[i] && is_drop(points_[i])) { pending_drop_flags_[i] = 1; forgetPoint_((int)i); }
  }
  template <class EFFrameT> void marginalizeFrame(EnergyFunctionalT* ef, EFFrameT* f) {
    int old_idx = -1, idx = 0;                             // idx counts the frames the prior still covers (sdso_abi.h)
    for (size_t k = 0; k < frames_.size(); k++) {
      if (frames_[k] == f) { old_idx = (int)k; break; }
      if (std::find(pending_rm_frames_.begin(), pending_rm_frames_.end(), (int)k) == pending_rm_frames_.end()) idx++;
    }
    if (old_idx < 0) throw Error("marginalizeFrame: the frame is not part of the uploaded window");
    const int left = nf_ - (int)pending_rm_frames_.size() - 1, m = dim_(left);
    std::vector<double> H((size_t)m * m), b(m);
    dev_.check(sdso_ba_marginalize_frame_dev(dev_.ctx(), win_, idx, H.data(), b.data()), "sdso_ba_marginalize_frame_dev");
    ef->HM.resize(m, m); ef->bM.resize(m);
    detail::fill(ef->bM, b.data(), m); detail::fill(ef->HM, H.data(), m, m);
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
  template <class SlotOf> void update(EnergyFunctionalT* ef, SlotOf slot_of) { update_(ef, slot_of, nullptr, 0); }
  template <class SlotOf, class FrameHessianT>
  std::vector<int> updateActivated(EnergyFunctionalT* ef, SlotOf slot_of, const std::vector<FrameHessianT*>& frameHessians, size_t n_records) {
    std::vector<const void*> act(frameHessians.begin(), frameHessians.end());
    return update_(ef, slot_of, &act, n_records);
  }
  // the index of ef frame `f` in the device window (after upload() / update()); -1: not part of it
  template <class EFFrameT> int frameIndex(const EFFrameT* f) const {
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
    F.bind(E);
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
    HM_.assign((size_t)dim_(nf_) * dim_(nf_), 0.0); bM_.assign(dim_(nf_), 0.0);   // (host copies of the prior: sized per window, filled by marginalizePointsF)
    clearPending_();
    window_serial_++;
    stateMoved_();
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
  std::vector<uint8_t> flag_decisions_;                    // sdso_ba_flag_points of the latest removeOutliers(), device point order
  bool flags_pending_ = false;
  int window_serial_ = 0, flags_serial_ = 0;               // upload() / update() count; the count the decisions were made at
  std::vector<int> pending_drop_res_, pending_rm_points_, pending_rm_frames_;
  std::vector<uint8_t> pending_drop_flags_;
  std::vector<const void*> frames_;                        // EFFrame* of the uploaded window, in order
  template <class MatXX, class VecX> void stitched_(int which, MatXX& H, VecX& b) {
    const int n = dim_(nf_);
    std::vector<double> Hs((size_t)n * n), bs(n);
    double* Hp[3] = {nullptr, nullptr, nullptr};
    double* bp[3] = {nullptr, nullptr, nullptr};
    Hp[which] = Hs.data(); bp[which] = bs.data();
    dev_.check(sdso_ba_get_stitched(dev_.ctx(), win_, Hp[0], bp[0], Hp[1], bp[1], Hp[2], bp[2]), "sdso_ba_get_stitched");
    H.resize(n, n); b.resize(n);
    detail::fill(b, bs.data(), n); detail::fill(H, Hs.data(), n, n);
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
  // a frame's, a point's and a residual's record as columns of the ABI's arrays: upload() fills one set for the window, update() one for its gains
  struct FrameCols {
    std::vector<double> evalPT, state, state_zero; std::vector<float> exposure, energyTH; std::vector<int> frameID, slots;
    void clear() { evalPT.clear(); state.clear(); state_zero.clear(); exposure.clear(); energyTH.clear(); frameID.clear(); slots.clear(); }
    template <class FrameHessianT, class SlotOf> void push(FrameHessianT* fh, SlotOf& slot_of) {
      const sdso_se3_t T = toAbi(fh->get_worldToCam_evalPT());
      evalPT.insert(evalPT.end(), T.R, T.R + 9); evalPT.insert(evalPT.end(), T.t, T.t + 3);
      for (int i = 0; i < 10; i++) { state.push_back(fh->get_state()[i]); state_zero.push_back(fh->get_state_zero()[i]); }
      exposure.push_back(fh->ab_exposure); energyTH.push_back(fh->frameEnergyTH); frameID.push_back(fh->frameID); slots.push_back(slot_of(fh));
    }
    // into sdso_ba_window_t or sdso_ba_window_edit_t: the two name the frame columns alike (the point and residual columns they do not)
    template <class AbiT> void bind(AbiT& W) const {
      W.evalPT = evalPT.data(); W.state = state.data(); W.state_zero = state_zero.data();
      W.ab_exposure = exposure.data(); W.frameEnergyTH = energyTH.data(); W.frameID = frameID.data(); W.frame_slot = slots.data();
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
  static int dim_(int nf) { return 8 * nf + 4; }           // the size of a window's system: CPARS + 8 per frame
  void stateMoved_() { lin_valid_ = app_valid_ = acc_valid_ = marg_valid_ = false; }   // the window changed, or a linearisation ran: nothing holds
  void marginalised_() { marg_valid_ = true; acc_valid_ = lin_valid_ = app_valid_ = false; }   // (it re-linearised its points)
  static void writeLastSystem_(EnergyFunctionalT* ef, const double* x, const double* HS, const double* bS, int n) {
    ef->lastX.resize(n); ef->lastbS.resize(n); ef->lastHS.resize(n, n);
    detail::fill(ef->lastX, x, n); detail::fill(ef->lastbS, bS, n); detail::fill(ef->lastHS, HS, n, n);
  }
  void reindex_() {                                        // points_ / residuals_ -> their index maps
    res_index_.clear(); point_index_.clear();
    for (size_t i = 0; i < residuals_.size(); i++) res_index_[residuals_[i]->data] = (int)i;
    for (size_t i = 0; i < points_.size(); i++) point_index_[points_[i]] = (int)i;
  }
  FrameCols up_frames_; PointCols up_points_; ResCols up_res_;   // upload()'s buffers, kept from call to call
  std::vector<double> HM_, bM_;
  std::vector<std::decay_t<decltype(std::declval<EnergyFunctionalT&>().frames[0]->points[0])>> points_;          // EFPoint*
  std::vector<std::decay_t<decltype(std::declval<EnergyFunctionalT&>().frames[0]->points[0]->residualsAll[0])>> residuals_;  // EFResidual*
};
}  // namespace sdso_shim
