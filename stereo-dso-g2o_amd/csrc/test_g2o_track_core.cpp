// csrc/g2o_track_core.h — one try of the fork-live trackNewestCoarse as a state machine over its evaluations — as a stand-alone program.
// The core is driven with closed-form evaluators (per level a quadratic in the translation and the affine pair with a Huber flattening and
// a Jacobian that may be reported too small, so that trials are rejected; a level whose cost does not move; a level whose cost rises
// on every trial; a level without points) and held, level by level, to g2o_lm::run (g2o_lm.h) on the very same callbacks: the
// iterations, the trials of each, lambda and chi2 after each, the stop reason and the estimate the level ends on, bit for bit.  Then what
// the core adds around the controller: the total_edges denominator, the events (order, at most five, recorded before the abort), the
// aborts, STEP4's verdicts, the evaluation counts.  Built and run plain and under the address / undefined-behaviour sanitizers by
// tests/test_g2o_track_core_cpu.py.
#define __host__
#define __device__
#include "g2o_track_core.h"
#include "g2o_lm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdso;
using g2o_track::Core;
using g2o_track::Eval;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

enum Kind { QUAD = 0, FLAT = 1, SPIKE = 2, EMPTY = 3 };

// the evaluators: residual k of level l is s[k] * (q[k] - target[k]) over q = {t0, t1, t2, a, b}
struct World {
  int kind[5] = {QUAD, QUAD, QUAD, QUAD, QUAD};
  int n[5] = {900, 500, 300, 130, 70}, edges[5] = {800, 450, 280, 120, 64};
  double jscale[5] = {1, 1, 1, 1, 1};          // the reported Jacobian over the true one: < 1 makes Gauss-Newton overshoot
  double target[5][5], s[5] = {3, 2, 4, 0.5, 0.25}, delta = 9;
  double floor_chi = 1000;                     // what no estimate removes: the second iteration of a converged level gains less than 1e-3 of it
  bool in_trial = false;                       // the caller's label of the pending request: a SPIKE level rises on every trial
  int calls = 0;
  long long points = 0;
  World() {
    for (int l = 0; l < 5; l++) { const double T[5] = {0.2 + 0.01 * l, -0.1, 0.35, 0.03, -1.5 + 0.1 * l}; for (int k = 0; k < 5; k++) target[l][k] = T[k]; }
  }
  static void q_of(const Se3& T, const double* aff, double* q) { q[0] = T.t[0]; q[1] = T.t[1]; q[2] = T.t[2]; q[3] = aff[0]; q[4] = aff[1]; }
  void answer(int l, int req, const Se3& T, const double* aff, Eval& E) {
    calls++; points += kind[l] == EMPTY ? 0 : n[l];
    std::memset(&E, 0, sizeof(E));
    if (req == g2o_track::REQ_CALCRES) {
      E.n_edges = kind[l] == EMPTY ? 0 : edges[l]; E.n_saturated = 3;
      E.flow[0] = l == 0 ? 1.25 : 0; E.flow[1] = 0; E.flow[2] = l == 0 ? 2.5 : 0;
      return;
    }
    if (kind[l] == EMPTY) return;
    if (kind[l] == FLAT) { E.sums[44] = 777; E.sums[45] = 555; return; }
    double q[5], J[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    q_of(T, aff, q);
    const int col[5] = {0, 1, 2, 6, 7};
    for (int k = 0; k < 5; k++) {
      const double e = s[k] * (q[k] - target[l][k]), e2 = e * e, dsqr = delta * delta;
      double rho0, rho1;
      if (e2 <= dsqr) { rho0 = e2; rho1 = 1; } else { const double a = std::sqrt(e2); rho0 = 2 * a * delta - dsqr; rho1 = delta / a; }
      for (int c = 0; c < 8; c++) J[c] = 0;
      J[col[k]] = s[k] * jscale[l];
      int i = 0;
      for (int r = 0; r < 8; r++) for (int c = r; c < 8; c++) E.sums[i++] += J[r] * rho1 * J[c];
      for (int r = 0; r < 8; r++) E.sums[36 + r] -= rho1 * J[r] * e;
      E.sums[44] += e2; E.sums[45] += rho0;
    }
    E.sums[44] += floor_chi; E.sums[45] += floor_chi;
    if (kind[l] == SPIKE && in_trial) { E.sums[44] += 1e6; E.sums[45] += 1e6; }
    if (req == g2o_track::REQ_ERRORS) for (int i = 0; i < 44; i++) E.sums[i] = 0;
  }
};

// one level as g2o_lm::run's problem, on the same evaluators and the same solve / update as the core's
struct LevelProb {
  World& W; int lvl;
  Se3 pose, trial_pose;
  double aff[2], affT[2], Hs[64], bs[8], x[8], work[80];
  int piv[8];
  LevelProb(World& w, int l, const Se3& T, const double* a) : W(w), lvl(l), pose(T), trial_pose(T) { aff[0] = affT[0] = a[0]; aff[1] = affT[1] = a[1]; }
  int build() {
    Eval E; W.answer(lvl, g2o_track::REQ_LINEARIZE, pose, aff, E);
    int k = 0;
    for (int r = 0; r < 8; r++) for (int c = r; c < 8; c++) { Hs[r * 8 + c] = E.sums[k]; Hs[c * 8 + r] = E.sums[k]; k++; }
    for (int r = 0; r < 8; r++) bs[r] = E.sums[36 + r];
    return 0;
  }
  int trial(double lambda, g2o_lm::TrialEval* t) {
    double A[64];
    for (int i = 0; i < 64; i++) A[i] = Hs[i];
    for (int r = 0; r < 8; r++) { A[r * 8 + r] = Hs[r * 8 + r] + lambda; x[r] = 0; }
    t->solved = solveLdltSmall(A, 8, 8, bs, x, work, piv);
    trial_pose = pose; affT[0] = aff[0]; affT[1] = aff[1];
    if (t->solved) { trial_pose = expSe3(x) * pose; affT[0] += x[6]; affT[1] += x[7]; }
    Eval E;
    W.in_trial = true; W.answer(lvl, g2o_track::REQ_ERRORS, trial_pose, affT, E); W.in_trial = false;
    t->chi2 = E.sums[45];
    t->scale = 0;
    for (int r = 0; r < 8; r++) t->scale += x[r] * (lambda * x[r] + bs[r]);
    return 0;
  }
  void accept() { pose = trial_pose; aff[0] = affT[0]; aff[1] = affT[1]; }
  int evaluate(double* chi) { Eval E; W.answer(lvl, g2o_track::REQ_ERRORS, pose, aff, E); *chi = E.sums[45]; return 0; }
};

static sdso_track_params_t params(int coarsest) {
  sdso_track_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.levels = coarsest + 1; p.coarsestLvl = coarsest;
  p.ref_exposure = 1; p.new_exposure = 1;
  for (int i = 0; i < 5; i++) p.minResForAbort[i] = NAN;
  p.coarseCutoffTH = 20; p.huberTH = 9;
  p.affineOptModeA = 1e12; p.affineOptModeB = 1e8;
  return p;
}

struct RefLevel { g2o_lm::Result R; Se3 pose; double aff[2]; double chi_end; };

// the levels one after the other through g2o_lm::run
static void reference(World& W, int coarsest, const sdso_se3_t& T0, const sdso_aff_t& a0, double lambda_init, RefLevel* out) {
  Se3 pose = se3_from_abi(T0);
  double aff[2] = {a0.a, a0.b};
  for (int l = coarsest; l >= 0; l--) {
    Eval E; W.answer(l, g2o_track::REQ_CALCRES, pose, aff, E);
    LevelProb P(W, l, pose, aff);
    double chi0; P.evaluate(&chi0);
    const g2o_lm::Params prm = {g2o_track::kIterations, lambda_init, g2o_track::kGainThreshold, g2o_track::kMaxTrials};
    if (g2o_lm::run(P, prm, chi0, &out[l].R) != 0) { std::printf("g2o_lm::run failed\n"); std::exit(2); }
    pose = P.pose; aff[0] = P.aff[0]; aff[1] = P.aff[1];
    out[l].pose = pose; out[l].aff[0] = aff[0]; out[l].aff[1] = aff[1]; out[l].chi_end = out[l].R.final_chi2;
  }
}

static void drive(Core& c, World& W) {
  double work[80]; int piv[8];
  W.calls = 0; W.points = 0;
  int guard = 0;
  while (!c.done && guard <= g2o_track::kMaxEvaluations) {
    Eval E;
    W.in_trial = c.phase == g2o_track::PH_TRIAL; W.answer(c.lvl, c.req, c.reqT, c.reqAff, E); W.in_trial = false;
    c.consume(E, work, piv);
    guard++;
  }
  CHECK(c.done && guard <= g2o_track::kMaxEvaluations);
  CHECK(c.out.evaluations == W.calls);
}

// the core's record of level l against g2o_lm::run's
static void same_level(const Core& c, int l, const RefLevel& r) {
  CHECK(c.out.iterations[l] == r.R.iterations);
  CHECK(c.stop_reason[l] == r.R.stop);
  for (int i = 0; i < r.R.iterations && i < g2o_track::kIterations; i++) {
    CHECK(c.trials[l][i] == r.R.trials[i]);
    CHECK(same(c.lambda_after[l][i], r.R.lambda[i]));
    CHECK(same(c.chi2_after[l][i], r.R.chi2[i]));
  }
}

int main() {
  sdso_se3_t T0;
  { const double xi[6] = {0.01, 0.02, -0.03, 0, 0, 0}; se3_to_abi(expSe3(xi), T0); }
  const sdso_aff_t a0 = {0.0, 0.0};
  {   // five plain levels: every level accepts its first trials; the second iteration gains nothing (exact quadratic): the gain stop
    World W;
    RefLevel ref[5];
    reference(W, 4, T0, a0, g2o_track::kLambdaInit, ref);
    Core c; c.init(params(4), W.n, T0, a0);
    drive(c, W);
    unsigned long long tot = 0;
    CHECK(c.trace.n == 5 && c.wrote_final && c.out.good == 1);
    for (int l = 4; l >= 0; l--) {
      same_level(c, l, ref[l]);
      CHECK(ref[l].R.iterations == 2 && ref[l].R.trials[0] == 1 && ref[l].R.stop == g2o_lm::STOP_GAIN);
      tot += (unsigned long long)W.edges[l];
      CHECK(same(c.out.lastResiduals[l], sqrtf((float)ref[l].chi_end / (float)tot)));       // the denominator runs over the levels so far
      CHECK(c.trace.lvl[4 - l] == l && same(c.trace.res[4 - l], c.out.lastResiduals[l]));   // the events: levels in descending order
      CHECK(same(c.trace.flow[4 - l][0], l == 0 ? 1.25 : 0.0) && same(c.trace.flow[4 - l][2], l == 0 ? 2.5 : 0.0));
    }
    CHECK(same(c.out.lastFlowIndicators[0], 1.25) && same(c.out.lastFlowIndicators[1], 0.0) && same(c.out.lastFlowIndicators[2], 2.5));
    CHECK(c.out.evaluations == 5 * (1 + 2 * 3) && c.out.point_evals == W.points);
    for (int i = 0; i < 3; i++) CHECK(same(c.T_final.t[i], ref[0].pose.t[i]));
    for (int i = 0; i < 9; i++) CHECK(same(c.T_final.R[i], ref[0].pose.R[i]));
    CHECK(same(c.aff_final.a, ref[0].aff[0]) && same(c.aff_final.b, ref[0].aff[1]));
    CHECK(std::fabs(c.T_final.t[0] - W.target[0][0]) < 1e-2 && std::fabs(c.aff_final.b - W.target[0][4]) < 5e-2);   // it converges
  }
  {   // a Jacobian reported at 0.3 of the true one on level 2: rejected trials, then an accepted one; rho == 0 on level 1 (a cost that does not move); ten
      // failed trials on level 3 (a cost that rises on every trial); level 0 without points
    World W;
    W.jscale[2] = 0.3; W.kind[1] = FLAT; W.kind[3] = SPIKE; W.kind[0] = EMPTY; W.n[0] = 0;
    RefLevel ref[5];
    reference(W, 3, T0, a0, g2o_track::kLambdaInit, ref);
    Core c; c.init(params(3), W.n, T0, a0);
    drive(c, W);
    for (int l = 3; l >= 0; l--) same_level(c, l, ref[l]);
    CHECK(ref[3].R.stop == g2o_lm::STOP_TRIALS && ref[3].R.trials[0] == 10 && ref[3].R.iterations == 1);
    CHECK(same(ref[3].R.lambda[0], 0.01 * std::pow(2.0, 55)));
    CHECK(ref[2].R.trials[0] > 1 && ref[2].R.trials[0] < 10 && ref[2].R.stop != g2o_lm::STOP_TRIALS);   // rejected, then accepted
    CHECK(ref[1].R.stop == g2o_lm::STOP_RHO_ZERO && ref[1].R.iterations == 1 && ref[1].R.trials[0] == 1);
    CHECK(ref[0].R.stop == g2o_lm::STOP_RHO_ZERO && ref[0].R.iterations == 1);                        // the level without points: x = 0, chi2 = 0
    // level 0: calcRes, the linearisation, one trial, the terminate action, the extra evaluation
    CHECK(c.out.evaluations == (1 + 1 + 10 + 1) + (1 + ref[2].R.trials[0] + ref[2].R.trials[1] + 2 * 2) + (1 + 1 + 1 + 1) + 5);
    CHECK(c.out.point_evals == W.points);
    CHECK(same(c.out.lastResiduals[1], sqrtf((float)555 / (float)(W.edges[3] + W.edges[2] + W.edges[1]))));
    CHECK(same(c.out.lastResiduals[0], sqrtf((float)0 / (float)(W.edges[3] + W.edges[2] + W.edges[1]))));   // no new edges: the earlier levels' count
    CHECK(c.trace.n == 4 && c.out.good == 1);
    {   // ... and the accepted trial of level 2 lowered the cost it started from (level 3 moved nothing: that start is the call's)
      Eval E0; const double aa[2] = {a0.a, a0.b};
      W.answer(2, g2o_track::REQ_ERRORS, se3_from_abi(T0), aa, E0);
      CHECK(ref[2].R.chi2[0] < E0.sums[45]);
    }
    // a try of empty levels alone: every residual is 0 / 0
    World Z;
    for (int l = 0; l < 5; l++) { Z.kind[l] = EMPTY; Z.n[l] = 0; }
    Core z; z.init(params(3), Z.n, T0, a0);
    drive(z, Z);
    CHECK(z.out.good == 1 && z.out.evaluations == 20 && z.trace.n == 4 && z.out.point_evals == 0);
    for (int l = 0; l < 4; l++) CHECK(z.out.iterations[l] == 1 && std::isnan(z.out.lastResiduals[l]));
    CHECK(std::isnan(z.out.lastResiduals[4]));
    for (int i = 0; i < 3; i++) CHECK(same(z.T_final.t[i], T0.t[i]));
  }
  {   // a lambda that stops being finite (only reachable from a larger lambda0 than the fork's: 0.01 * 2^55 is finite)
    World W;
    W.kind[2] = SPIKE;
    RefLevel ref[5];
    reference(W, 2, T0, a0, 1e300, ref);
    Core c; c.init(params(2), W.n, T0, a0);
    c.lambda_init = 1e300;
    drive(c, W);
    for (int l = 2; l >= 0; l--) same_level(c, l, ref[l]);
    CHECK(ref[2].R.stop == g2o_lm::STOP_LAMBDA && ref[2].R.trials[0] < 10 && !std::isfinite(ref[2].R.lambda[0]) && c.out.iterations[2] == 1);
  }
  {   // aborts: at the coarsest level and at a middle one; the event is recorded before the test, the references stay untouched
    for (int at = 3; at >= 1; at -= 2) {
      World W;
      RefLevel ref[5];
      reference(W, 3, T0, a0, g2o_track::kLambdaInit, ref);
      sdso_track_params_t p = params(3);
      Core free_run; free_run.init(p, W.n, T0, a0);
      drive(free_run, W);
      for (int l = 0; l < 4; l++) p.minResForAbort[l] = 1e9;
      p.minResForAbort[at] = free_run.out.lastResiduals[at] / 1.5 * 0.999;     // res > 1.5 * bound by 0.1 %
      Core c; c.init(p, W.n, T0, a0);
      drive(c, W);
      CHECK(c.done && !c.wrote_final && c.out.good == 0);
      CHECK(c.trace.n == 3 - at + 1 && c.trace.lvl[c.trace.n - 1] == at);
      for (int e = 0; e < c.trace.n; e++) CHECK(same(c.trace.res[e], free_run.trace.res[e]) && c.trace.lvl[e] == free_run.trace.lvl[e]);
      for (int l = 0; l < at; l++) CHECK(std::isnan(c.out.lastResiduals[l]) && c.out.iterations[l] == 0);
      CHECK(same(c.out.lastResiduals[at], free_run.out.lastResiduals[at]));
      CHECK(std::memcmp(&c.T_final, &T0, sizeof(T0)) == 0 && c.aff_final.a == a0.a && c.aff_final.b == a0.b);
      p.minResForAbort[at] = free_run.out.lastResiduals[at] / 1.5 * 1.001;     // just inside the bound: no abort
      Core d; d.init(p, W.n, T0, a0);
      drive(d, W);
      CHECK(d.wrote_final && d.trace.n == 4);
    }
  }
  {   // STEP4's verdicts (:1050-1068)
    World W;
    auto run_with = [&](double modeA, double modeB, float ref_exp, float new_exp) {
      sdso_track_params_t p = params(1);
      p.affineOptModeA = modeA; p.affineOptModeB = modeB; p.ref_exposure = ref_exp; p.new_exposure = new_exp;
      Core c; c.init(p, W.n, T0, a0);
      drive(c, W);
      CHECK(c.wrote_final && c.trace.n == 2);
      return c;
    };
    const Core ok = run_with(1e12, 1e8, 1, 1);
    CHECK(ok.out.good == 1 && std::fabs(ok.aff_final.b + 1.5) < 0.1);
    for (int l = 0; l < 2; l++) W.target[l][3] = 1.5;                 // |a| > 1.2 with the affine a optimised: not good, a is handed out
    const Core bigA = run_with(1e12, 1e8, 1, 1);
    CHECK(bigA.out.good == 0 && bigA.aff_final.a > 1.2);
    for (int l = 0; l < 2; l++) { W.target[l][3] = 0.03; W.target[l][4] = -250; }   // |b| > 200
    const Core bigB = run_with(1e12, 1e8, 1, 1);
    CHECK(bigB.out.good == 0 && bigB.aff_final.b < -200);
    const Core relB = run_with(1e12, 0, 1, 1);                        // mode B == 0: the relative b is tested
    CHECK(relB.out.good == 0);
    for (int l = 0; l < 2; l++) W.target[l][4] = -1.5;
    const Core relA = run_with(0, 1e8, 1, 100);                       // mode A == 0: |log(relative a)| = log(100) > 1.5
    CHECK(relA.out.good == 0);
    const Core relOk = run_with(0, 0, 1, 2);                          // log(2) < 1.5
    CHECK(relOk.out.good == 1 && relOk.aff_final.a != 0);
    const Core fixed = run_with(-1, -1, 1, 1);                        // negative modes: the pair is handed out as zero
    CHECK(fixed.out.good == 1 && fixed.aff_final.a == 0 && fixed.aff_final.b == 0);
  }
  {   // the request record: the vertices' estimates travel, the level's constants stay
    World W;
    sdso_track_params_t p = params(2);
    p.ref_exposure = 2; p.new_exposure = 3; p.ref_aff_g2l.a = 0.01; p.ref_aff_g2l.b = 4;
    const sdso_aff_t a1 = {0.05, -2.0};
    Core c; c.init(p, W.n, T0, a1);
    sdso_g2o_track_eval_t ev;
    std::memset(&ev, 0, sizeof(ev));
    ev.lvl = 2; ev.cutoffTH = 20; ev.Ki[4] = 7;
    g2o_track::fill_request(c, ev);
    double a2[2];
    affFromTo(2, 3, 0.01, 4, 0.05, -2.0, a2);
    CHECK(c.req == g2o_track::REQ_CALCRES && c.lvl == 2 && ev.lvl == 2 && ev.cutoffTH == 20 && ev.Ki[4] == 7);
    CHECK(std::memcmp(ev.R, T0.R, 72) == 0 && std::memcmp(ev.t, T0.t, 24) == 0 && ev.ab[0] == (float)a2[0] && ev.ab[1] == (float)a2[1]);
  }
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("g2o_track_core ok\n");
  return 0;
}
