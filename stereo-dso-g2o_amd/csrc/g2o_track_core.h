// One try of CoarseTracker::trackNewestCoarse as the fork runs it (CoarseTracker.cpp:827-1069), cut at its evaluations and stated once
// for host and device: "here are the sums of the evaluation you asked for — tell me the next one, or that you are done".  k_g2o_track_lm
// (g2o_track_lm.hip) walks it on thread 0 of a workgroup between two barriers; csrc/test_g2o_track_core.cpp walks it on a CPU over
// closed-form evaluators and holds it to g2o_lm::run (g2o_lm.h).  Plain C++ under SDSO_HD: no ctx, no HIP call.
//
// It is sdso_g2o_track_newest_coarse (g2o_factors.hip) with the calls turned inside out, and holds exactly what that body holds:
//   - levels coarsestLvl .. 0, each opened by a calcRes at the CALL'S INITIAL pose (refToNew_current never moves, :880, :894): the cull
//     tables of every level are the caller's constants, only the vertices' estimates travel with a request;
//   - g2o's Levenberg-Marquardt as g2o_lm.h states it ("parity unpinned"): lambda0 0.01, 2 iterations, at most 10 trials, computeScale
//     + 1e-3, the 1/3 .. 2/3 factor, the terminate action's fresh evaluation with its gain threshold 1e-3, and the extra evaluation of a
//     level without points;
//   - the update exp(x) * pose, a += x6, b += x7 (dso_g2o_vertex.cpp:15-18, :30-40);
//   - lastResiduals[lvl] = sqrtf((float)chi2 / total_edges) with total_edges running over the levels so far (:1029), the flow indicators
//     of the level's calcRes, the abort test (:1032), STEP4 (:1050-1068);
//   - the evaluations / point_evals / iterations[] conventions of sdso_track_result_t.
// The fork-live body never repeats a level (levelCutoffRepeat stays 1, :891-904): a try has at most five events.  An event is recorded
// where lastResiduals[lvl] is written, BEFORE the abort test, as LmCore::finish_level (tracker_lm_core.h) does.
//
// Three kinds of request.  A trial and the terminate action read activeRobustChi2 only, so they ask for the errors alone; the
// linearisation at the head of an iteration asks for the whole system.
#pragma once
#include <cmath>
#include "host_math.h"

namespace sdso {
namespace g2o_track {

constexpr int kIterations = 2;             // maxIterations {2,2,2,2,2} (:861)
constexpr double kLambdaInit = 0.01;       // setUserLambdaInit(0.01), :839-840
constexpr double kGainThreshold = 1e-3;    // SparseOptimizerTerminateAction::setGainThreshold
constexpr int kMaxTrials = 10;             // _maxTrialsAfterFailure
// a level: its calcRes, per iteration the linearisation, the trials and the terminate action's evaluation, the extra evaluation
constexpr int kMaxEvaluations = 5 * (1 + kIterations * (2 + kMaxTrials) + 1);
constexpr int kSums = 36 + 8 + 2;          // upper triangle of H, b, {chi2, robust chi2}

enum Request { REQ_CALCRES = 0, REQ_LINEARIZE = 1, REQ_ERRORS = 2 };
enum Phase { PH_CALCRES = 0, PH_BUILD = 1, PH_TRIAL = 2, PH_EVAL = 3, PH_EXTRA = 4 };
enum Stop { STOP_ITERATIONS = 0, STOP_GAIN = 1, STOP_TRIALS = 2, STOP_RHO_ZERO = 3, STOP_LAMBDA = 4 };   // g2o_lm::Stop's values

// what an evaluation hands back
struct Eval {
  double sums[kSums];        // REQ_LINEARIZE: all of it; REQ_ERRORS: [44], [45] only; REQ_CALCRES: not read
  int n_edges, n_saturated;  // REQ_CALCRES: numTermsInE, numSaturated
  double flow[3];            // REQ_CALCRES: res[2..4] of calcRes (:783-789)
};

struct Core {
  // ---- the call
  sdso_track_params_t p;
  int n[5];                  // pc_n
  // ---- the estimate and the tentative one
  Se3 pose, trial;
  double aff[2], affT[2];
  // ---- g2o's LM on the current level
  double Hs[64], Hd[8], bs[8], x[8];   // the system as linearised (Hd: its diagonal), the increment
  double lambda_init;                  // kLambdaInit (a member so that the CPU test can reach the exit of a lambda that stops being finite)
  double lambda, ni, lastChi, currentChi, rho, chi;
  int it, qmax;
  bool stop, ok, solved;
  // ---- the level
  int lvl, phase;
  unsigned long long total_edges;
  double resOld[3];
  // ---- the request
  int req;
  Se3 reqT;
  double reqAff[2];
  bool done;
  // ---- what the call leaves
  sdso_track_result_t out;
  sdso_track_trace_t trace;
  bool wrote_final;
  sdso_se3_t T_final;
  sdso_aff_t aff_final;
  // ---- the controller's record per level and iteration (g2o_lm::Result's members; the CPU test reads them)
  int trials[5][kIterations], stop_reason[5];
  double lambda_after[5][kIterations], chi2_after[5][kIterations];

  SDSO_HD void init(const sdso_track_params_t& prm, const int* pc_n, const sdso_se3_t& T0, const sdso_aff_t& aff0) {
    p = prm;
    for (int l = 0; l < 5; l++) {
      n[l] = pc_n[l]; stop_reason[l] = STOP_ITERATIONS;
      for (int i = 0; i < kIterations; i++) { trials[l][i] = 0; lambda_after[l][i] = 0; chi2_after[l][i] = 0; }
    }
    pose = se3_from_abi(T0); trial = pose;
    aff[0] = aff0.a; aff[1] = aff0.b; affT[0] = aff[0]; affT[1] = aff[1];
    for (int i = 0; i < 64; i++) Hs[i] = 0;
    for (int i = 0; i < 8; i++) { Hd[i] = 0; bs[i] = 0; x[i] = 0; }
    lambda_init = kLambdaInit;
    lambda = 0; ni = 2; lastChi = 0; currentChi = 0; rho = 0; chi = 0;
    it = 0; qmax = 0; stop = false; ok = true; solved = false;
    total_edges = 0;
    for (int i = 0; i < 3; i++) resOld[i] = 0;
    done = false; wrote_final = false;
    T_final = T0; aff_final = aff0;
    out.good = 0; out.evaluations = 0; out.point_evals = 0;          // CoarseTracker.cpp:846-856
    for (int i = 0; i < 5; i++) { out.lastResiduals[i] = NAN; out.iterations[i] = 0; }
    for (int i = 0; i < 3; i++) out.lastFlowIndicators[i] = 1000;
    trace.n = 0;
    for (int e = 0; e < SDSO_TRACK_MAX_EVENTS; e++) { trace.lvl[e] = 0; trace.res[e] = 0; for (int k = 0; k < 3; k++) trace.flow[e][k] = 0; }
    lvl = p.coarsestLvl;
    start_level();
  }

  SDSO_HD void request(int kind, const Se3& T, const double* a) {
    req = kind; reqT = T; reqAff[0] = a[0]; reqAff[1] = a[1];
    out.evaluations++; out.point_evals += n[lvl];
  }
  SDSO_HD void start_level() { phase = PH_CALCRES; request(REQ_CALCRES, pose, aff); }

  // solve (H + lambda I) x = b, form the tentative estimate, ask for its errors
  SDSO_HD void propose(double* work, int* piv) {
    for (int r = 0; r < 8; r++) { x[r] = 0; Hs[r * 8 + r] = Hd[r] + lambda; }
    solved = solveLdltSmall(Hs, 8, 8, bs, x, work, piv);
    trial = pose; affT[0] = aff[0]; affT[1] = aff[1];
    if (solved) {
      trial = expSe3(x) * pose;                                      // VertexSE3PoseDSO::oplusImpl, dso_g2o_vertex.cpp:15-18
      affT[0] += x[6]; affT[1] += x[7];                              // VertexPhotometricDSO::oplusImpl, :30-40
    }
    phase = PH_TRIAL;
    request(REQ_ERRORS, trial, affT);
  }

  // the head of an iteration, or what follows the last one
  SDSO_HD void next_iteration() {
    if (it < kIterations && !stop && ok) { phase = PH_BUILD; request(REQ_LINEARIZE, pose, aff); }
    else if (kIterations == 0 || n[lvl] == 0) { phase = PH_EXTRA; request(REQ_ERRORS, pose, aff); }
    else finish_level();
  }

  SDSO_HD void finish_level() {
    out.lastResiduals[lvl] = sqrtf((float)chi / (float)total_edges);   // :1029
    for (int k = 0; k < 3; k++) out.lastFlowIndicators[k] = resOld[k]; // :1030
    if (trace.n < SDSO_TRACK_MAX_EVENTS) {
      const int e = trace.n++;
      trace.lvl[e] = lvl; trace.res[e] = out.lastResiduals[lvl];
      for (int k = 0; k < 3; k++) trace.flow[e][k] = out.lastFlowIndicators[k];
    }
    if (out.lastResiduals[lvl] > 1.5 * p.minResForAbort[lvl]) { done = true; return; }   // :1032-1033: the references stay untouched
    lvl--;
    if (lvl >= 0) { start_level(); return; }
    // STEP4, :1044-1068
    done = true; wrote_final = true;
    se3_to_abi(pose, T_final);
    aff_final.a = aff[0]; aff_final.b = aff[1];
    if ((p.affineOptModeA != 0 && (fabsf((float)aff_final.a) > 1.2)) || (p.affineOptModeB != 0 && (fabsf((float)aff_final.b) > 200))) return;
    double relAff[2];
    affFromTo(p.ref_exposure, p.new_exposure, p.ref_aff_g2l.a, p.ref_aff_g2l.b, aff_final.a, aff_final.b, relAff);
    if ((p.affineOptModeA == 0 && (fabsf(logf((float)relAff[0])) > 1.5)) || (p.affineOptModeB == 0 && (fabsf((float)relAff[1]) > 200))) return;
    if (p.affineOptModeA < 0) aff_final.a = 0;
    if (p.affineOptModeB < 0) aff_final.b = 0;
    out.good = 1;
  }

  // E: the evaluation of the pending request.  work: 80 doubles, piv: 8 ints of the caller's (LDS on the device).
  SDSO_HD void consume(const Eval& E, double* work, int* piv) {
    if (phase == PH_CALCRES) {
      total_edges += (unsigned long long)E.n_edges;
      for (int k = 0; k < 3; k++) resOld[k] = E.flow[k];
      it = 0; stop = false; ok = true; lambda = 0; ni = 2; lastChi = 0; chi = 0;
      next_iteration();
    } else if (phase == PH_BUILD) {
      int k = 0;
      for (int r = 0; r < 8; r++)
        for (int c = r; c < 8; c++) { Hs[r * 8 + c] = E.sums[k]; Hs[c * 8 + r] = E.sums[k]; k++; }
      for (int r = 0; r < 8; r++) { bs[r] = E.sums[36 + r]; Hd[r] = Hs[r * 8 + r]; }
      chi = E.sums[45];
      currentChi = chi;
      if (it == 0) { lambda = lambda_init; ni = 2; }
      rho = 0; qmax = 0;
      propose(work, piv);
    } else if (phase == PH_TRIAL) {
      chi = E.sums[45];
      const double tempChi = solved ? chi : 1.7976931348623157e308;
      rho = currentChi - tempChi;
      double scale = 0;
      for (int r = 0; r < 8; r++) scale += x[r] * (lambda * x[r] + bs[r]);   // computeScale
      scale += 1e-3;
      rho /= scale;
      bool broke = false;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        lambda *= (1. / 3. > alpha ? 1. / 3. : alpha);
        ni = 2;
        currentChi = tempChi;
        pose = trial; aff[0] = affT[0]; aff[1] = affT[1];
      } else {
        lambda *= ni;
        ni *= 2;
        if (!std::isfinite(lambda)) broke = true;
      }
      if (!broke) qmax++;
      if (!broke && rho < 0 && qmax < kMaxTrials) { propose(work, piv); return; }
      if (!std::isfinite(lambda)) { ok = false; stop_reason[lvl] = STOP_LAMBDA; }
      else if (rho == 0) { ok = false; stop_reason[lvl] = STOP_RHO_ZERO; }
      else if (qmax == kMaxTrials) { ok = false; stop_reason[lvl] = STOP_TRIALS; }
      phase = PH_EVAL;
      request(REQ_ERRORS, pose, aff);                                // terminate action: computeActiveErrors at the current estimate
    } else if (phase == PH_EVAL) {
      chi = E.sums[45];
      trials[lvl][it] = qmax; lambda_after[lvl][it] = lambda; chi2_after[lvl][it] = chi;
      out.iterations[lvl]++;
      if (it == 0) lastChi = chi;
      else {
        const double gain = (lastChi - chi) / chi;
        lastChi = chi;
        if (gain >= 0 && gain < kGainThreshold) { stop = true; if (ok) stop_reason[lvl] = STOP_GAIN; }
      }
      it++;
      next_iteration();
    } else {                                                         // PH_EXTRA
      chi = E.sums[45];
      finish_level();
    }
  }
};

// the vertices' estimates of the pending request into the level's evaluation record: `ev` holds the level's constants (camera, Ki, the
// cull tables at the call's initial pose, thresholds) and keeps them
SDSO_HD inline void fill_request(const Core& c, sdso_g2o_track_eval_t& ev) {
  for (int i = 0; i < 9; i++) ev.R[i] = c.reqT.R[i];
  for (int i = 0; i < 3; i++) ev.t[i] = c.reqT.t[i];
  double a2[2];
  affFromTo(c.p.ref_exposure, c.p.new_exposure, c.p.ref_aff_g2l.a, c.p.ref_aff_g2l.b, c.reqAff[0], c.reqAff[1], a2);
  ev.ab[0] = (float)a2[0]; ev.ab[1] = (float)a2[1];
}

}  // namespace g2o_track
}  // namespace sdso
