// What the fork-live window optimiser decides between its evaluations (FullSystemOptimize.cpp:402-868 as sdso_g2o_lba_optimize restates
// it), stated once for host and device.  It is to g2o_lm.h what g2o_track_core.h is: g2o_lm::run cut at the evaluations, plus the two
// pieces of LbaProblem::trial (g2o_lba_opt.hip) that run on the host there — the assembly of the block-arrow reduced system and its
// solve.  k_lbar_ctl (g2o_lba_resident.hip) walks it as a single workgroup between the wide kernels; csrc/test_g2o_lba_core.cpp walks it
// on a CPU and holds it to g2o_lm::run and to LbaProblem::trial's assembly with solveLdlt, bit for bit.
// Plain C++ under SDSO_HD: no ctx, no HIP call.
//
// Lm — the controller.  `phase` says which launches of the fixed schedule still have work:
//   PH_INIT        the build-time evaluation is under way (set by whoever creates the record)   -> start()
//   PH_HEAD        an iteration begins: linearise, then PH_TRIAL's steps
//   PH_TRIAL       Schur complement at `lambda`, solve, tentative estimate          -> trial_proposed()
//   PH_TRIAL_EVAL  evaluate the tentative estimate                                  -> trial_result()
//   PH_TERM_EVAL   the terminate action: evaluate the current estimate              -> eval_result()
//   PH_DONE        nothing is left; every later launch returns at once
//
// The parallel pieces take a `Par`: tid() / nt() number the calling threads, sync() is their barrier.  Every thread of the group calls
// them with the same arguments; what a thread computes for an element does not depend on nt(), so Serial (one thread, here) and a
// workgroup (the device) give the same bits.
#pragma once
#include <cmath>
#include "host_math.h"

namespace sdso {
namespace g2o_lba {

constexpr int kEnt = 91;            // upper triangle of a host's 13 x 13 [pose 6 | photometric 2 | camera 4 | error]
constexpr int kNMax = 68;           // 8 hosts x 8 + the camera's 4
constexpr int kMaxRecorded = 64;    // SDSO_G2O_LBA_MAX_RECORDED
enum Stop { STOP_ITERATIONS = 0, STOP_GAIN = 1, STOP_TRIALS = 2, STOP_RHO_ZERO = 3, STOP_LAMBDA = 4 };   // g2o_lm::Stop's values
enum Phase { PH_INIT = 0, PH_HEAD = 1, PH_TRIAL = 2, PH_TRIAL_EVAL = 3, PH_TERM_EVAL = 4, PH_DONE = 5 };

struct Serial {
  SDSO_HD int tid() const { return 0; }
  SDSO_HD int nt() const { return 1; }
  SDSO_HD void sync() const {}
};

struct Lm {
  int max_iterations, max_trials;
  double lambda_init, gain_threshold;
  double lambda, ni, lastChi, currentChi, chi, rho;
  int it, qmax, stop_flag, ok, phase;
  int accepted;                     // trial_result's verdict on the tentative estimate
  // what the run leaves (g2o_lm::Result's members)
  int iterations, stop;
  int trials[kMaxRecorded];
  double lambda_rec[kMaxRecorded], chi2_rec[kMaxRecorded];
  double final_chi2;

  SDSO_HD void begin_iteration() {
    currentChi = chi;
    if (it == 0) { lambda = lambda_init; ni = 2; }
    rho = 0; qmax = 0;
    phase = PH_HEAD;
  }
  // chi2_initial: activeRobustChi2 of the build-time evaluation; any_active: the active set is not empty (an empty one runs nothing)
  SDSO_HD void start(int max_it, double lam0, double gain_thr, int max_tr, double chi2_initial, bool any_active) {
    max_iterations = max_it; max_trials = max_tr; lambda_init = lam0; gain_threshold = gain_thr;
    lambda = 0; ni = 2; lastChi = 0; currentChi = 0; chi = chi2_initial; rho = 0;
    it = 0; qmax = 0; stop_flag = 0; ok = 1; accepted = 0;
    iterations = 0; stop = STOP_ITERATIONS; final_chi2 = chi2_initial;
    for (int i = 0; i < kMaxRecorded; i++) { trials[i] = 0; lambda_rec[i] = 0; chi2_rec[i] = 0; }
    if (any_active && it < max_iterations) begin_iteration();
    else phase = PH_DONE;
  }
  SDSO_HD void trial_proposed() { phase = PH_TRIAL_EVAL; }
  // the tentative estimate's evaluation: solved — the solver's verdict (false: chi2 is not read); scale — computeScale over ALL unknowns
  SDSO_HD void trial_result(bool solved, double chi2, double scale) {
    const double tempChi = solved ? chi2 : 1.7976931348623157e308;
    rho = currentChi - tempChi;
    rho /= scale + 1e-3;
    bool broke = false;
    accepted = 0;
    if (rho > 0 && std::isfinite(tempChi)) {
      double alpha = 1. - pow((2 * rho - 1), 3);
      alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
      lambda *= (1. / 3. > alpha ? 1. / 3. : alpha);
      ni = 2;
      currentChi = tempChi;
      accepted = 1;
    } else {
      lambda *= ni;
      ni *= 2;
      if (!std::isfinite(lambda)) broke = true;
    }
    if (!broke) qmax++;
    if (!broke && rho < 0 && qmax < max_trials) { phase = PH_TRIAL; return; }
    if (!std::isfinite(lambda)) { ok = 0; stop = STOP_LAMBDA; }
    else if (rho == 0) { ok = 0; stop = STOP_RHO_ZERO; }
    else if (qmax == max_trials) { ok = 0; stop = STOP_TRIALS; }
    phase = PH_TERM_EVAL;
  }
  // the terminate action's evaluation at the current estimate
  SDSO_HD void eval_result(double chi2) {
    chi = chi2;
    if (it < kMaxRecorded) { trials[it] = qmax; lambda_rec[it] = lambda; chi2_rec[it] = chi; }
    iterations++;
    final_chi2 = chi;
    if (it == 0) lastChi = chi;
    else {
      const double gain = (lastChi - chi) / chi;
      lastChi = chi;
      if (gain >= 0 && gain < gain_threshold) { stop_flag = 1; if (ok) stop = STOP_GAIN; }
    }
    it++;
    if (it < max_iterations && !stop_flag && ok) begin_iteration();
    else phase = PH_DONE;
  }
};

// entry `ent` of the upper triangle, row-major: (i, j), i <= j < 13
SDSO_HD inline void entry_ij(int ent, int& i, int& j) {
  i = 0;
  int k = ent;
  while (k >= 13 - i) { k -= 13 - i; i++; }
  j = i + k;
}

// hosts with an active edge in frame order; returns their number
SDSO_HD inline int make_slots(const int* n_active_host, int nf, int* slot) {
  int nh = 0;
  for (int h = 0; h < nf; h++) slot[h] = n_active_host[h] > 0 ? nh++ : -1;
  return nh;
}

// The reduced system as LbaProblem::trial assembles it: A, S — per host the folded quadratic form and its Schur complement at lambda
// (kEnt each, by frame index); hosts with a slot in frame order, then the camera; lambda on every diagonal.  H: n x n with row stride
// kNMax, both triangles; bfull, bred: n.  An entry is owned by one thread, which adds the hosts' terms in frame order.
template <class Par>
SDSO_HD inline void assemble(const Par& par, const double* A, const double* S, const int* slot, int nf, int nh, double lambda,
                             double* H, double* bfull, double* bred) {
  const int n = 8 * nh + 4;
  for (int k = par.tid(); k < n * kNMax; k += par.nt()) H[k] = 0;
  for (int k = par.tid(); k < n; k += par.nt()) { bfull[k] = 0; bred[k] = 0; }
  par.sync();
  for (int ent = par.tid(); ent < kEnt; ent += par.nt()) {
    int i, j;
    entry_ij(ent, i, j);
    for (int h = 0; h < nf; h++) {
      if (slot[h] < 0) continue;
      const int gi = i < 8 ? 8 * slot[h] + i : 8 * nh + (i - 8);
      const double a = A[h * kEnt + ent], s = S[h * kEnt + ent];
      if (j == 12) {
        if (i < 12) { bfull[gi] -= a; bred[gi] += -a - s; }
        continue;
      }
      const int gj = j < 8 ? 8 * slot[h] + j : 8 * nh + (j - 8);
      const double v = a - s;
      H[gi * kNMax + gj] += v;
      if (gi != gj) H[gj * kNMax + gi] += v;
    }
  }
  par.sync();
  for (int k = par.tid(); k < n; k += par.nt()) H[k * kNMax + k] += lambda;
  par.sync();
}

// x = H^-1 rhs by solveLdlt's algorithm (host_math.h), operation for operation.  The pivot of every step is a function of the input
// diagonal alone, so one thread finds the whole sequence first (the exchanges on a copy of the diagonal only); the exchanges of rows
// and columns, the division, the right-looking update of the lower triangle and its mirror then run step by step as solveLdlt has
// them, spread over the threads — every element sees the arithmetic solveLdlt gives it, whichever thread owns it.  H (n x n, row
// stride kNMax, both triangles) is destroyed.  D, y, d0: n doubles each; p, pivs: n ints each; flag: one int.
// Returns on every thread: no zero pivot and x finite.
template <class Par>
SDSO_HD inline bool solve(const Par& par, int n, double* H, const double* rhs, double* x, double* D, double* y, double* d0, int* p, int* pivs,
                          int* flag) {
  double* A = H;
  if (par.tid() == 0) {
    for (int i = 0; i < n; i++) { p[i] = i; d0[i] = A[i * kNMax + i]; }
    for (int k = 0; k < n; k++) {
      int piv = k;
      double best = fabs(d0[k]);
      int i = k + 1;
      for (; i + 7 < n; i += 8) {                    // (eight loads in flight; the comparisons keep their order)
        double v[8];
        for (int q = 0; q < 8; q++) v[q] = fabs(d0[i + q]);
        for (int q = 0; q < 8; q++)
          if (v[q] > best) { best = v[q]; piv = i + q; }
      }
      for (; i < n; i++)
        if (fabs(d0[i]) > best) { best = fabs(d0[i]); piv = i; }
      pivs[k] = piv;
      if (piv != k) {
        const int t = p[k]; p[k] = p[piv]; p[piv] = t;
        const double td = d0[k]; d0[k] = d0[piv]; d0[piv] = td;
      }
    }
    *flag = 1;
  }
  par.sync();
  // the threads as a tw x th grid over the trailing block: rows by ty, columns by tx
  const int tw = par.nt() >= 16 ? 16 : 1, th = par.nt() / tw, tx = par.tid() % tw, ty = par.tid() / tw;
  for (int k = 0; k < n; k++) {
    const int piv = pivs[k];
    if (piv != k) {                                  // (uniform)
      for (int j = par.tid(); j < n; j += par.nt()) { const double t = A[k * kNMax + j]; A[k * kNMax + j] = A[piv * kNMax + j]; A[piv * kNMax + j] = t; }
      par.sync();
      for (int i = par.tid(); i < n; i += par.nt()) { const double t = A[i * kNMax + k]; A[i * kNMax + k] = A[i * kNMax + piv]; A[i * kNMax + piv] = t; }
      par.sync();
    }
    const double d = A[k * kNMax + k];             // (nothing below writes (k, k))
    if (par.tid() == 0) { D[k] = d; if (d == 0.0) *flag = 0; }
    if (d == 0.0) continue;                          // (uniform) a zero pivot leaves its column undivided
    for (int i = k + 1 + par.tid(); i < n; i += par.nt()) A[i * kNMax + k] /= d;
    par.sync();
    // A(i, j) -= l d A(j, k) over the lower triangle, and its mirror at once: column k, all this reads besides the element itself, is
    // not written here, and (j, i) belongs to the thread that owns (i, j)
    if (ty < th)
      for (int i = k + 1 + ty; i < n; i += th) {
        const double l = A[i * kNMax + k];
        if (l == 0.0) continue;
        for (int j = k + 1 + tx; j <= i; j += tw) {
          const double v = A[i * kNMax + j] - l * d * A[j * kNMax + k];
          A[i * kNMax + j] = v;
          if (j < i) A[j * kNMax + i] = v;
        }
      }
    par.sync();
  }
  for (int i = par.tid(); i < n; i += par.nt()) y[i] = rhs[p[i]];
  par.sync();
  // L y' = y, column by column: row i subtracts its terms in the order j = 0 .. i - 1, as solveLdlt's row loop does
  for (int j = 0; j < n; j++) {
    const double yj = y[j];
    for (int i = j + 1 + par.tid(); i < n; i += par.nt()) y[i] -= A[i * kNMax + j] * yj;
    par.sync();
  }
  if (par.tid() == 0) {
    for (int i = 0; i < n; i++) y[i] = D[i] != 0.0 ? y[i] / D[i] : 0.0;
    // L^T x = y': row i subtracts in the order j = i + 1 .. n - 1 and needs every later x first: one thread, eight products in flight
    for (int i = n - 1; i >= 0; i--) {
      double s = y[i];
      int j = i + 1;
      for (; j + 7 < n; j += 8) {
        double pr[8];
        for (int q = 0; q < 8; q++) pr[q] = A[(j + q) * kNMax + i] * y[j + q];
        for (int q = 0; q < 8; q++) s -= pr[q];
      }
      for (; j < n; j++) s -= A[j * kNMax + i] * y[j];
      y[i] = s;
    }
    for (int i = 0; i < n; i++) { x[p[i]] = y[i]; if (!std::isfinite(y[i])) *flag = 0; }
  }
  par.sync();
  return *flag != 0;
}

// computeScale's part over the pose, photometric and camera unknowns, in index order
SDSO_HD inline double scale_of(const double* x, const double* bfull, int n, double lambda) {
  double s = 0;
  for (int k = 0; k < n; k++) s += x[k] * (lambda * x[k] + bfull[k]);
  return s;
}

// One pair of the float tables (dso_g2o_edge.cpp:25-28, :86-91) in LbaProblem::tables' operation order: {R 9, t 3} of Ttw[tg] * Twh[h] and
// the affine pair, cast to float
SDSO_HD inline void pair_table(const Se3& Ttw, const Se3& Twh, float exp_h, float exp_t, double aff_a, double aff_b, double tgt_a, double tgt_b,
                               float* R, float* t, float* ab) {
  const Se3 Tth = Ttw * Twh;
  for (int k = 0; k < 9; k++) R[k] = (float)Tth.R[k];
  for (int k = 0; k < 3; k++) t[k] = (float)Tth.t[k];
  double o[2];
  affFromTo(exp_h, exp_t, aff_a, aff_b, tgt_a, tgt_b, o);
  ab[0] = (float)o[0]; ab[1] = (float)o[1];
}

}  // namespace g2o_lba
}  // namespace sdso
