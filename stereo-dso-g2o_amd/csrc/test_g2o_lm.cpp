// csrc/g2o_lm.h — g2o's Levenberg-Marquardt control as the fork's window optimiser and tracker run it — as a stand-alone program:
// a small dense least-squares problem that really converges, and scripted chi2 sequences that walk every exit of the controller
// (accept, reject, the trial cap, rho == 0, a lambda that stops being finite, the gain stop, the iteration cap, a failing solver,
// a failing step).  Built and run plain and under the address / undefined-behaviour sanitizers by tests/test_g2o_lm_cpu.py.
#include "g2o_lm.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdso::g2o_lm;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
static bool near(double a, double b, double rel = 1e-12) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

// min |A x - y|^2 over 3 unknowns, 6 rows
struct Dense3 {
  double A[6][3] = {{1, 2, 0}, {0, 1, 3}, {2, 0, 1}, {1, 1, 1}, {3, -1, 0}, {0, 2, -2}};
  double y[6] = {1, 2, 3, 4, 5, 6};
  double x[3] = {0, 0, 0}, xt[3], H[3][3], b[3];
  int builds = 0, trials = 0, accepts = 0, evals = 0;
  double chi_at(const double* v) const {
    double s = 0;
    for (int r = 0; r < 6; r++) { double e = -y[r]; for (int k = 0; k < 3; k++) e += A[r][k] * v[k]; s += e * e; }
    return s;
  }
  int build() {
    builds++;
    for (int i = 0; i < 3; i++) {
      b[i] = 0;
      for (int j = 0; j < 3; j++) { H[i][j] = 0; for (int r = 0; r < 6; r++) H[i][j] += A[r][i] * A[r][j]; }
      for (int r = 0; r < 6; r++) { double e = -y[r]; for (int k = 0; k < 3; k++) e += A[r][k] * x[k]; b[i] -= A[r][i] * e; }
    }
    return 0;
  }
  int trial(double lambda, TrialEval* t) {
    trials++;
    double M[3][4];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) M[i][j] = H[i][j] + (i == j ? lambda : 0); M[i][3] = b[i]; }
    for (int k = 0; k < 3; k++)
      for (int i = k + 1; i < 3; i++) { const double f = M[i][k] / M[k][k]; for (int j = k; j < 4; j++) M[i][j] -= f * M[k][j]; }
    double dx[3];
    for (int i = 2; i >= 0; i--) { double s = M[i][3]; for (int j = i + 1; j < 3; j++) s -= M[i][j] * dx[j]; dx[i] = s / M[i][i]; }
    t->solved = true;
    t->scale = 0;
    for (int k = 0; k < 3; k++) { xt[k] = x[k] + dx[k]; t->scale += dx[k] * (lambda * dx[k] + b[k]); }
    t->chi2 = chi_at(xt);
    return 0;
  }
  void accept() { accepts++; for (int k = 0; k < 3; k++) x[k] = xt[k]; }
  int evaluate(double* chi) { evals++; *chi = chi_at(x); return 0; }
};

// a problem that replays scripts: trial k returns trial_chi[k] / trial_scale[k], evaluation k returns eval_chi[k]
struct Script {
  std::vector<double> trial_chi, trial_scale, eval_chi, lambdas;
  std::vector<int> solved;
  size_t t = 0, e = 0;
  int builds = 0, accepts = 0, fail_build_at = -1, fail_trial_at = -1;
  int build() { return builds++ == fail_build_at ? -7 : 0; }
  int trial(double lambda, TrialEval* out) {
    if ((int)t == fail_trial_at) return -9;
    if (t >= trial_chi.size()) { std::printf("script ran out of trials\n"); std::exit(2); }
    lambdas.push_back(lambda);
    out->solved = solved.empty() ? true : solved[t] != 0;
    out->chi2 = trial_chi[t];
    out->scale = trial_scale.empty() ? 1.0 : trial_scale[t];
    t++;
    return 0;
  }
  void accept() { accepts++; }
  int evaluate(double* chi) {
    if (e >= eval_chi.size()) { std::printf("script ran out of evaluations\n"); std::exit(2); }
    *chi = eval_chi[e++];
    return 0;
  }
};

int main() {
  const Params prm = {10, 0.1, 1e-3, 10};
  {   // the dense problem converges to the normal-equation solution and stops on the gain
    Dense3 P;
    Result R;
    CHECK(run(P, prm, P.chi_at(P.x), &R) == 0);
    CHECK(R.stop == STOP_GAIN && R.iterations >= 2 && R.iterations < 10);
    CHECK(P.builds == R.iterations && P.evals == R.iterations && P.accepts == R.iterations && P.trials == R.iterations);
    for (int i = 0; i < R.iterations; i++) CHECK(R.trials[i] == 1);
    CHECK(near(R.lambda[0], 0.1 / 3));                      // a step that does what the model predicts: the 1/3 factor
    for (int i = 1; i < R.iterations; i++) CHECK(R.chi2[i] <= R.chi2[i - 1]);
    P.build();
    for (int k = 0; k < 3; k++) CHECK(std::fabs(P.b[k]) < 1e-2);
    CHECK(near(R.final_chi2, P.chi_at(P.x)));
  }
  {   // zero iterations: nothing is called
    Script S;
    Result R;
    Params p0 = prm; p0.max_iterations = 0;
    CHECK(run(S, p0, 42.0, &R) == 0);
    CHECK(R.iterations == 0 && R.stop == STOP_ITERATIONS && R.final_chi2 == 42.0 && S.builds == 0 && S.t == 0 && S.e == 0);
  }
  {   // two rejected trials, then an accepted one; lambda * 2 * 4, then the 2/3 cap; then the iteration cap
    Script S;
    S.trial_chi = {120, 110, 90, 80};       // chi0 = 100
    S.trial_scale = {1, 1, 20 - 1e-3, 10 - 1e-3};
    S.eval_chi = {90, 80};
    Result R;
    Params p = prm; p.max_iterations = 2;
    CHECK(run(S, p, 100.0, &R) == 0);
    CHECK(R.iterations == 2 && R.stop == STOP_ITERATIONS && R.trials[0] == 3 && R.trials[1] == 1 && S.accepts == 2);
    CHECK(near(S.lambdas[0], 0.1) && near(S.lambdas[1], 0.2) && near(S.lambdas[2], 0.8));
    // rho = 10 / 20 = 0.5: alpha = 1 - 0 = 1 -> min(1, 2/3)
    CHECK(near(R.lambda[0], 0.8 * 2. / 3.));
    // second iteration: rho = (90 - 80) / 10 = 1: alpha = 0 -> the 1/3 floor; nu was reset (the first trial's lambda is the iteration's)
    CHECK(near(S.lambdas[3], R.lambda[0]) && near(R.lambda[1], R.lambda[0] / 3));
    CHECK(R.chi2[0] == 90 && R.chi2[1] == 80 && R.final_chi2 == 80);
  }
  {   // the trial cap: ten rejections, lambda * 2^(1 + 2 + ... + 10)
    Script S;
    S.trial_chi.assign(10, 200.0);
    S.eval_chi = {100};
    Result R;
    CHECK(run(S, prm, 100.0, &R) == 0);
    CHECK(R.iterations == 1 && R.stop == STOP_TRIALS && R.trials[0] == 10 && S.accepts == 0 && S.builds == 1);
    CHECK(near(R.lambda[0], 0.1 * std::pow(2.0, 55)));
  }
  {   // an ACCEPTED tenth trial ends the run as well (g2o tests qmax == maxTrials after the loop)
    Script S;
    S.trial_chi.assign(9, 200.0);
    S.trial_chi.push_back(50.0);
    S.eval_chi = {50};
    Result R;
    CHECK(run(S, prm, 100.0, &R) == 0);
    CHECK(R.iterations == 1 && R.stop == STOP_TRIALS && S.accepts == 1 && R.final_chi2 == 50);
  }
  {   // rho == 0: the trial changes nothing
    Script S;
    S.trial_chi = {100};
    S.eval_chi = {100};
    Result R;
    CHECK(run(S, prm, 100.0, &R) == 0);
    CHECK(R.iterations == 1 && R.stop == STOP_RHO_ZERO && R.trials[0] == 1 && S.accepts == 0 && near(R.lambda[0], 0.2));
  }
  {   // lambda stops being finite
    Script S;
    S.trial_chi.assign(10, 200.0);
    S.eval_chi = {100};
    Result R;
    Params p = prm; p.lambda_init = 1e300;
    CHECK(run(S, p, 100.0, &R) == 0);
    CHECK(R.iterations == 1 && R.stop == STOP_LAMBDA && !std::isfinite(R.lambda[0]) && R.trials[0] < 10 && S.accepts == 0);
  }
  {   // a failing solver counts as a rejected trial whatever chi2 says
    Script S;
    S.trial_chi = {1, 90, 89.99};
    S.solved = {0, 1, 1};
    S.eval_chi = {90, 89.99};
    Result R;
    CHECK(run(S, prm, 100.0, &R) == 0);
    CHECK(R.trials[0] == 2 && R.trials[1] == 1 && S.accepts == 2 && R.stop == STOP_GAIN && R.iterations == 2);
  }
  {   // the gain stop: 0 <= (lastChi - chi) / chi < 1e-3 after the second iteration; a negative gain does not stop
    Script S;
    S.trial_chi = {90, 95, 94.95};
    S.eval_chi = {90, 95, 94.95};          // the second evaluation is WORSE (gain < 0): goes on; the third gains 5e-4: stops
    S.trial_scale = {5, -5, 0.05};          // rho > 0 each time
    Result R;
    CHECK(run(S, prm, 100.0, &R) == 0);
    CHECK(R.iterations == 3 && R.stop == STOP_GAIN && R.final_chi2 == 94.95);
  }
  {   // a failing step ends the run with its code
    Script S;
    S.trial_chi = {90};
    S.eval_chi = {90};
    S.fail_build_at = 1;
    Result R;
    CHECK(run(S, prm, 100.0, &R) == -7);
    Script T;
    T.fail_trial_at = 0;
    CHECK(run(T, prm, 100.0, &R) == -9);
  }
  {   // more iterations than are recorded: counted, run, not written past the arrays
    Script S;
    const int n = kMaxRecorded + 6;
    for (int i = 0; i < n; i++) { S.trial_chi.push_back(1000.0 - 10 * (i + 1)); S.eval_chi.push_back(1000.0 - 10 * (i + 1)); }
    S.trial_scale.assign(n, 10 - 1e-3);
    Result R;
    Params p = prm; p.max_iterations = n;
    CHECK(run(S, p, 1000.0, &R) == 0);
    CHECK(R.iterations == n && R.stop == STOP_ITERATIONS && R.trials[kMaxRecorded - 1] == 1 && R.final_chi2 == 1000.0 - 10 * n);
  }
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("g2o_lm ok\n");
  return 0;
}
