// csrc/g2o_lba_core.h — what the fork-live window optimiser decides between its evaluations, the text k_lbar_ctl walks on the device —
// as a stand-alone program.
//   1. Lm, driven over closed-form evaluators (a dense least-squares problem that converges; scripted chi2 sequences that reach every
//      exit), against g2o_lm::run (g2o_lm.h) on the very same evaluators: the calls in their order with their lambdas, the iterations, the
//      trials, lambda and chi2 of each, the stop reason, the final chi2 — bit for bit.  All five stop reasons.
//   2. assemble + solve against LbaProblem::trial's assembly (g2o_lba_opt.hip, restated below line for line) with solveLdlt
//      (host_math.h), on random block-arrow systems: 1..8 frames, some without a slot, lambda 1e-9 .. 1e8, columns scaled over four
//      decades.  The solver is solveLdlt's algorithm, so x and the verdict are compared bit for bit.  The systems are SPD by construction
//      (a quadratic form minus its Schur complement at lambda > 0); their condition numbers are printed (Jacobi eigenvalues, symEigen).
//      A singular system (lambda 0, a host whose terms are all zero) checks the zero-pivot verdict.
// Built and run plain and under the address / undefined-behaviour sanitizers by tests/test_g2o_lba_core_cpu.py.
#define __host__
#define __device__
#include "g2o_lba_core.h"
#include "g2o_lm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdso;
using g2o_lba::Lm;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// ---------------------------------------------------------------------------------------------- 1. the controller
struct Call { int kind; double lambda; };   // 0 build, 1 trial (its lambda), 2 accept, 3 evaluate
// min |A x - y|^2 over 3 unknowns with a Jacobian reported too small by `jscale`: Gauss-Newton overshoots and trials are rejected
struct Dense3 {
  double A[6][3] = {{1, 2, 0}, {0, 1, 3}, {2, 0, 1}, {1, 1, 1}, {3, -1, 0}, {0, 2, -2}};
  double y[6] = {1, 2, 3, 4, 5, 6};
  double x[3] = {0, 0, 0}, xt[3], H[3][3], b[3], jscale = 1;
  std::vector<Call> log;
  double chi_at(const double* v) const {
    double s = 0;
    for (int r = 0; r < 6; r++) { double e = -y[r]; for (int k = 0; k < 3; k++) e += A[r][k] * v[k]; s += e * e; }
    return s;
  }
  int build() {
    log.push_back({0, 0});
    for (int i = 0; i < 3; i++) {
      b[i] = 0;
      for (int j = 0; j < 3; j++) { H[i][j] = 0; for (int r = 0; r < 6; r++) H[i][j] += jscale * A[r][i] * jscale * A[r][j]; }
      for (int r = 0; r < 6; r++) { double e = -y[r]; for (int k = 0; k < 3; k++) e += A[r][k] * x[k]; b[i] -= jscale * A[r][i] * e; }
    }
    return 0;
  }
  int trial(double lambda, g2o_lm::TrialEval* t) {
    log.push_back({1, lambda});
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
  void accept() { log.push_back({2, 0}); for (int k = 0; k < 3; k++) x[k] = xt[k]; }
  int evaluate(double* chi) { log.push_back({3, 0}); *chi = chi_at(x); return 0; }
};
// replays scripts: trial k returns trial_chi[k] / trial_scale[k] / solved[k], evaluation k returns eval_chi[k]
struct Script {
  std::vector<double> trial_chi, trial_scale, eval_chi;
  std::vector<int> solved;
  size_t t = 0, e = 0;
  std::vector<Call> log;
  int build() { log.push_back({0, 0}); return 0; }
  int trial(double lambda, g2o_lm::TrialEval* out) {
    if (t >= trial_chi.size()) { std::printf("script ran out of trials\n"); std::exit(2); }
    log.push_back({1, lambda});
    out->solved = solved.empty() ? true : solved[t] != 0;
    out->chi2 = trial_chi[t];
    out->scale = trial_scale.empty() ? 1.0 : trial_scale[t];
    t++;
    return 0;
  }
  void accept() { log.push_back({2, 0}); }
  int evaluate(double* chi) {
    if (e >= eval_chi.size()) { std::printf("script ran out of evaluations\n"); std::exit(2); }
    log.push_back({3, 0});
    *chi = eval_chi[e++];
    return 0;
  }
};

// the schedule of g2o_lba_resident.hip on a CPU: what each phase asks for, answered by the problem's callbacks
template <class P>
static void drive(P& prob, const g2o_lm::Params& prm, double chi0, bool any_active, Lm& lm) {
  lm.start(prm.max_iterations, prm.lambda_init, prm.gain_threshold, prm.max_trials, chi0, any_active);
  g2o_lm::TrialEval t;
  long guard = 0;
  while (lm.phase != g2o_lba::PH_DONE && guard++ < 1000000) {
    if (lm.phase == g2o_lba::PH_HEAD || lm.phase == g2o_lba::PH_TRIAL) {
      if (lm.phase == g2o_lba::PH_HEAD) prob.build();
      t = g2o_lm::TrialEval();
      prob.trial(lm.lambda, &t);
      lm.trial_proposed();
    } else if (lm.phase == g2o_lba::PH_TRIAL_EVAL) {
      lm.trial_result(t.solved, t.chi2, t.scale);
      if (lm.accepted) prob.accept();
    } else {
      double chi = 0;
      prob.evaluate(&chi);
      lm.eval_result(chi);
    }
  }
  CHECK(lm.phase == g2o_lba::PH_DONE);
}

template <class P>
static int both(const P& proto, const g2o_lm::Params& prm, double chi0, const char* what) {
  P a = proto, b = proto;
  g2o_lm::Result R;
  CHECK(g2o_lm::run(a, prm, chi0, &R) == 0);
  Lm lm;
  std::memset(&lm, 0xab, sizeof(lm));            // start() sets every field it reads
  drive(b, prm, chi0, true, lm);
  const int before = g_fail;
  CHECK(a.log.size() == b.log.size());
  for (size_t i = 0; i < a.log.size() && i < b.log.size(); i++) CHECK(a.log[i].kind == b.log[i].kind && same(a.log[i].lambda, b.log[i].lambda));
  CHECK(R.iterations == lm.iterations && R.stop == lm.stop && same(R.final_chi2, lm.final_chi2));
  for (int i = 0; i < g2o_lm::kMaxRecorded; i++) CHECK(R.trials[i] == lm.trials[i] && same(R.lambda[i], lm.lambda_rec[i]) && same(R.chi2[i], lm.chi2_rec[i]));
  std::printf("%-28s iterations %d stop %d calls %zu%s\n", what, R.iterations, R.stop, a.log.size(), g_fail == before ? "" : "  MISMATCH");
  return R.stop;
}

static void test_controller() {
  const g2o_lm::Params prm = {10, 0.1, 1e-3, 10};
  bool seen[5] = {false, false, false, false, false};
  {
    Dense3 P;
    seen[both(P, prm, P.chi_at(P.x), "dense, converges")] = true;
    P.jscale = 0.45;                              // overshoots: rejected trials on the way
    g2o_lm::Params p = prm; p.max_iterations = 25; p.lambda_init = 1e-4;
    seen[both(P, p, P.chi_at(P.x), "dense, overshooting")] = true;
    p.max_iterations = 2;
    seen[both(P, p, P.chi_at(P.x), "dense, two iterations")] = true;
    p.max_iterations = 0;
    seen[both(P, p, P.chi_at(P.x), "zero iterations")] = true;
  }
  {   // two rejected trials, then an accepted one; then the iteration cap
    Script S;
    S.trial_chi = {120, 110, 90, 80}; S.trial_scale = {1, 1, 20 - 1e-3, 10 - 1e-3}; S.eval_chi = {90, 80};
    g2o_lm::Params p = prm; p.max_iterations = 2;
    CHECK(both(S, p, 100.0, "script, iteration cap") == g2o_lm::STOP_ITERATIONS);
    seen[g2o_lm::STOP_ITERATIONS] = true;
  }
  {   // the gain stop
    Script S;
    S.trial_chi = {90, 89.99}; S.trial_scale = {9, 0.009}; S.eval_chi = {90, 89.99};
    CHECK(both(S, prm, 100.0, "script, gain") == g2o_lm::STOP_GAIN);
    seen[g2o_lm::STOP_GAIN] = true;
  }
  {   // the trial cap, with a max_trials that is not g2o's
    Script S;
    S.trial_chi.assign(4, 200.0); S.eval_chi = {100};
    g2o_lm::Params p = prm; p.max_trials = 4;
    CHECK(both(S, p, 100.0, "script, trial cap") == g2o_lm::STOP_TRIALS);
    seen[g2o_lm::STOP_TRIALS] = true;
  }
  {   // a trial that changes nothing: rho == 0
    Script S;
    S.trial_chi = {100}; S.eval_chi = {100};
    CHECK(both(S, prm, 100.0, "script, rho == 0") == g2o_lm::STOP_RHO_ZERO);
    seen[g2o_lm::STOP_RHO_ZERO] = true;
  }
  {   // a lambda that stops being finite on the second rejection
    Script S;
    S.trial_chi = {200, 200}; S.eval_chi = {100};
    g2o_lm::Params p = prm; p.lambda_init = 1e308;
    CHECK(both(S, p, 100.0, "script, lambda") == g2o_lm::STOP_LAMBDA);
    seen[g2o_lm::STOP_LAMBDA] = true;
  }
  {   // a solver that fails once: the trial counts as rejected with DBL_MAX, the next one is accepted
    Script S;
    S.trial_chi = {1, 90, 85}; S.solved = {0, 1, 1}; S.trial_scale = {1, 5, 5}; S.eval_chi = {90, 85};
    g2o_lm::Params p = prm; p.max_iterations = 2;
    both(S, p, 100.0, "script, solver fails");
  }
  for (int k = 0; k < 5; k++) CHECK(seen[k]);
  {   // an empty active set runs nothing
    Script S;
    Lm lm;
    drive(S, prm, 0.0, false, lm);
    CHECK(lm.iterations == 0 && lm.stop == g2o_lba::STOP_ITERATIONS && S.log.empty() && lm.final_chi2 == 0.0);
  }
}

// ---------------------------------------------------------------------------------------------- 2. the reduced system
static unsigned long long g_seed = 0x9e3779b97f4a7c15ull;
static double rnd() {   // (-1, 1)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_seed >> 11) / 9007199254740992.0) * 2 - 1;
}

// LbaProblem::trial's assembly (g2o_lba_opt.hip), line for line, over Dense / std::vector
static void assemble_ref(const double (*A)[g2o_lba::kEnt], const double (*S)[g2o_lba::kEnt], const int* slot, int nf, int nh, double lambda, Dense& Hr,
                         std::vector<double>& bfull, std::vector<double>& bred) {
  const int n = 8 * nh + 4;
  Hr = Dense(n);
  bfull.assign(n, 0.0); bred.assign(n, 0.0);
  for (int h = 0; h < nf; h++) {
    if (slot[h] < 0) continue;
    int ent = 0;
    for (int i = 0; i < 13; i++)
      for (int j = i; j < 13; j++, ent++) {
        const int gi = i < 8 ? 8 * slot[h] + i : 8 * nh + (i - 8);
        if (j == 12) {
          if (i < 12) { bfull[gi] -= A[h][ent]; bred[gi] += -A[h][ent] - S[h][ent]; }
          continue;
        }
        const int gj = j < 8 ? 8 * slot[h] + j : 8 * nh + (j - 8);
        const double v = A[h][ent] - S[h][ent];
        Hr(gi, gj) += v;
        if (gi != gj) Hr(gj, gi) += v;
      }
  }
  for (int k = 0; k < n; k++) Hr(k, k) += lambda;
}

static void test_system() {
  double cond_min = 1e300, cond_max = 0;
  int systems = 0;
  const double lambdas[] = {1e-9, 1e-6, 1e-3, 0.1, 1.0, 1e2, 1e5, 1e8};
  for (int nf = 1; nf <= 8; nf++)
    for (int rep = 0; rep < 6; rep++)
      for (double lambda : lambdas) {
        if (rep >= 2 && lambda != lambdas[(rep + nf) % 8]) continue;   // every lambda on two windows per nf, one lambda on the others
        static double A[8][g2o_lba::kEnt], S[8][g2o_lba::kEnt];
        int cnt[8], slot[8];
        double cs[13];
        for (int k = 0; k < 12; k++) cs[k] = std::pow(10.0, 2 * rnd());   // the columns' scales: four decades
        cs[12] = 3;
        for (int h = 0; h < nf; h++) {
          cnt[h] = (rep % 3 == 1 && nf > 1 && h % 3 == 1) ? 0 : 30 + (int)(20 * (rnd() + 1));   // some hosts have no active edge
          for (int e = 0; e < g2o_lba::kEnt; e++) { A[h][e] = 0; S[h][e] = 0; }
          for (int ed = 0; ed < cnt[h]; ed++) {
            double row[8][13], jd[8], rec[13] = {0}, hll = 0;
            for (int r = 0; r < 8; r++) { for (int k = 0; k < 13; k++) row[r][k] = cs[k] * rnd(); jd[r] = 2 * rnd(); }
            for (int k = 0; k < 12; k++) for (int r = 0; r < 8; r++) rec[k] += row[r][k] * jd[r];
            for (int r = 0; r < 8; r++) { rec[12] -= jd[r] * row[r][12]; hll += jd[r] * jd[r]; }
            int ent = 0;
            for (int i = 0; i < 13; i++)
              for (int j = i; j < 13; j++, ent++) {
                for (int r = 0; r < 8; r++) A[h][ent] += row[r][i] * row[r][j];
                S[h][ent] += (rec[i] * (1. / (hll + lambda))) * rec[j];
              }
          }
        }
        const int nh = g2o_lba::make_slots(cnt, nf, slot);
        const int n = 8 * nh + 4;
        Dense Hr;
        std::vector<double> bfull, bred, xr;
        assemble_ref(A, S, slot, nf, nh, lambda, Hr, bfull, bred);
        const bool ok_ref = solveLdlt(Hr, bred, xr);
        static double H[g2o_lba::kNMax * g2o_lba::kNMax];
        double bf[g2o_lba::kNMax], br[g2o_lba::kNMax], x[g2o_lba::kNMax], D[g2o_lba::kNMax], y[g2o_lba::kNMax], d0[g2o_lba::kNMax];
        int p[g2o_lba::kNMax], pivs[g2o_lba::kNMax], flag = -1;
        const g2o_lba::Serial par;
        g2o_lba::assemble(par, &A[0][0], &S[0][0], slot, nf, nh, lambda, H, bf, br);
        bool eq = true;
        for (int i = 0; i < n; i++) {
          eq = eq && same(bf[i], bfull[i]) && same(br[i], bred[i]);
          for (int j = 0; j < n; j++) eq = eq && same(H[i * g2o_lba::kNMax + j], Hr(i, j));
        }
        CHECK(eq);
        std::vector<double> w;
        Dense V;
        symEigen(Hr, w, V);
        double lo = 1e300, hi = 0;
        for (double v : w) { lo = std::min(lo, v); hi = std::max(hi, v); }
        CHECK(lo > 0);                                    // SPD
        cond_min = std::min(cond_min, hi / lo); cond_max = std::max(cond_max, hi / lo);
        const bool ok = g2o_lba::solve(par, n, H, br, x, D, y, d0, p, pivs, &flag);
        CHECK(ok == ok_ref && ok);
        bool xeq = true;
        for (int i = 0; i < n; i++) xeq = xeq && same(x[i], xr[i]);
        CHECK(xeq);
        double sref = 0;
        for (int k = 0; k < n; k++) sref += xr[k] * (lambda * xr[k] + bfull[k]);
        CHECK(same(sref, g2o_lba::scale_of(x, bf, n, lambda)));
        systems++;
      }
  std::printf("%d block-arrow systems, condition numbers %.3g .. %.3g: assembly, x, verdict and scale equal solveLdlt's bit for bit\n", systems, cond_min, cond_max);
  CHECK(cond_max > 1e8);
  {   // singular: lambda 0 and a host whose terms are all zero — a zero pivot, the verdict is false on both sides and x agrees
    static double A[8][g2o_lba::kEnt], S[8][g2o_lba::kEnt];
    for (int h = 0; h < 2; h++) for (int e = 0; e < g2o_lba::kEnt; e++) { A[h][e] = 0; S[h][e] = 0; }
    int ent = 0;
    for (int i = 0; i < 13; i++) for (int j = i; j < 13; j++, ent++) A[0][ent] = i == j ? 2.0 + i : 0.125;
    const int slot[2] = {0, 1};
    Dense Hr;
    std::vector<double> bfull, bred, xr;
    assemble_ref(A, S, slot, 2, 2, 0.0, Hr, bfull, bred);
    const bool ok_ref = solveLdlt(Hr, bred, xr);
    static double H[g2o_lba::kNMax * g2o_lba::kNMax];
    double bf[g2o_lba::kNMax], br[g2o_lba::kNMax], x[g2o_lba::kNMax], D[g2o_lba::kNMax], y[g2o_lba::kNMax], d0[g2o_lba::kNMax];
    int p[g2o_lba::kNMax], pivs[g2o_lba::kNMax], flag = -1;
    const g2o_lba::Serial par;
    g2o_lba::assemble(par, &A[0][0], &S[0][0], slot, 2, 2, 0.0, H, bf, br);
    const bool ok = g2o_lba::solve(par, 20, H, br, x, D, y, d0, p, pivs, &flag);
    CHECK(!ok && !ok_ref);
    for (int i = 0; i < 20; i++) CHECK(same(x[i], xr[i]));
  }
  {   // the pair table is LbaProblem::tables' text: the Se3 product and affFromTo, cast to float
    Se3 Ttw, Twh;
    const double xi[6] = {0.1, -0.2, 0.05, 0.02, -0.01, 0.03}, xj[6] = {-0.3, 0.1, 0.2, -0.02, 0.04, 0.01};
    Ttw = expSe3(xi); Twh = expSe3(xj);
    float R[9], t[3], ab[2];
    g2o_lba::pair_table(Ttw, Twh, 0.8f, 1.1f, 0.03, -2.0, -0.01, 1.5, R, t, ab);
    const Se3 T = Ttw * Twh;
    double o[2];
    affFromTo(0.8f, 1.1f, 0.03, -2.0, -0.01, 1.5, o);
    for (int k = 0; k < 9; k++) CHECK(R[k] == (float)T.R[k]);
    for (int k = 0; k < 3; k++) CHECK(t[k] == (float)T.t[k]);
    CHECK(ab[0] == (float)o[0] && ab[1] == (float)o[1]);
  }
}

int main() {
  test_controller();
  test_system();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("g2o_lba_core ok\n");
  return 0;
}
