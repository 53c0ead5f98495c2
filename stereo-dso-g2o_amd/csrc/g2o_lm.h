// g2o's Levenberg-Marquardt control, stated once: OptimizationAlgorithmLevenberg::solve around SparseOptimizer::optimize with a
// SparseOptimizerTerminateAction, as the fork runs it for the window (FullSystemOptimize.cpp:420-433, :587-590) and for the tracker
// (CoarseTracker.cpp:839-840).  g2o is neither vendored nor version-pinned by the reference tree (CMakeLists.txt:47-58): this is a
// restatement of its published algorithm, "parity unpinned", in the very form sdso_g2o_track_newest_coarse has it (g2o_factors.hip).
//
// Plain C++: no ctx, no HIP.  The problem P supplies four steps, each returning 0 or an error code that ends the run at once:
//   int build()                                    linearise at the current estimate (linearizeOplus + the quadratic form)
//   int trial(double lambda, TrialEval* t)         solve (H + lambda I) x = b, form the tentative estimate current (+) x, evaluate it:
//                                                    t->solved  the solver's verdict (false: chi2 is not read)
//                                                    t->chi2    activeRobustChi2 at the tentative estimate
//                                                    t->scale   computeScale: sum over ALL unknowns of x_k (lambda x_k + b_k)
//   void accept()                                  the tentative estimate becomes the current one (a rejected one is simply dropped)
//   int evaluate(double* chi2)                     computeActiveErrors at the current estimate -> activeRobustChi2
// The caller has evaluated the initial estimate itself and passes that chi2.
#pragma once
#include <algorithm>
#include <cmath>

namespace sdso {
namespace g2o_lm {

enum Stop { STOP_ITERATIONS = 0, STOP_GAIN = 1, STOP_TRIALS = 2, STOP_RHO_ZERO = 3, STOP_LAMBDA = 4 };
constexpr int kMaxRecorded = 64;   // iterations whose trials / lambda / chi2 are recorded (later ones still run and count)

struct Params {
  int max_iterations;
  double lambda_init;       // setUserLambdaInit
  double gain_threshold;    // SparseOptimizerTerminateAction::setGainThreshold
  int max_trials;           // _maxTrialsAfterFailure (10)
};
struct TrialEval {
  bool solved = false;
  double chi2 = 0, scale = 0;
};
struct Result {
  int iterations = 0, stop = STOP_ITERATIONS;
  int trials[kMaxRecorded];
  double lambda[kMaxRecorded], chi2[kMaxRecorded];
  double final_chi2 = 0;    // of the last evaluation: the estimate the run ends on
};

template <class P>
int run(P& prob, const Params& prm, double chi2_initial, Result* out) {
  Result& R = *out;
  R.iterations = 0; R.stop = STOP_ITERATIONS; R.final_chi2 = chi2_initial;
  for (int i = 0; i < kMaxRecorded; i++) { R.trials[i] = 0; R.lambda[i] = 0; R.chi2[i] = 0; }
  double lambda = 0, ni = 2, lastChi = 0, chi = chi2_initial;
  bool stop = false, ok = true;
  int rc;
  for (int it = 0; it < prm.max_iterations && !stop && ok; it++) {
    if ((rc = prob.build())) return rc;
    double currentChi = chi;
    if (it == 0) { lambda = prm.lambda_init; ni = 2; }
    double rho = 0;
    int qmax = 0;
    do {
      TrialEval t;
      if ((rc = prob.trial(lambda, &t))) return rc;
      const double tempChi = t.solved ? t.chi2 : 1.7976931348623157e308;
      rho = currentChi - tempChi;
      rho /= t.scale + 1e-3;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
        prob.accept();
      } else {
        lambda *= ni;
        ni *= 2;
        if (!std::isfinite(lambda)) break;
      }
      qmax++;
    } while (rho < 0 && qmax < prm.max_trials);
    if (!std::isfinite(lambda)) { ok = false; R.stop = STOP_LAMBDA; }
    else if (rho == 0) { ok = false; R.stop = STOP_RHO_ZERO; }
    else if (qmax == prm.max_trials) { ok = false; R.stop = STOP_TRIALS; }
    if ((rc = prob.evaluate(&chi))) return rc;   // terminate action: computeActiveErrors at the current estimate
    if (it < kMaxRecorded) { R.trials[it] = qmax; R.lambda[it] = lambda; R.chi2[it] = chi; }
    R.iterations++;
    R.final_chi2 = chi;
    if (it == 0) lastChi = chi;
    else {
      const double gain = (lastChi - chi) / chi;
      lastChi = chi;
      if (gain >= 0 && gain < prm.gain_threshold) { stop = true; if (ok) R.stop = STOP_GAIN; }
    }
  }
  return 0;
}

}  // namespace g2o_lm
}  // namespace sdso
