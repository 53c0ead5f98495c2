// BA host API, part 3 (included by ba.hip): the per-window step calls (FullSystem::linearizeAll, EnergyFunctional::accumulate*,
// solveSystemF, resubstituteF, calc*Energy) and the getters, sdso_ba_linearize ... sdso_ba_get_deltas, sdso_ba_get_state,
// sdso_ba_get_post_state, sdso_ba_get_counts, ba_ref_view, ba_window_points.
extern "C" int sdso_ba_accum_floats(int nf) { return (int)acc_floats(nf); }

namespace sdso {
// a per-residual device array (pair-sorted, `width` entries per residual) into the window's residual order: one blocking copy
template <class T> static int fetch_to_window_order(sdso_ctx* ctx, const BaWindowDev* W, const T* dsrc, int width, T* dst) {
  const int nr = W->d.nr;
  if (!nr) return SDSO_OK;
  std::vector<T> tmp((size_t)nr * width);
  SDSO_HIP(ctx, hipMemcpy(tmp.data(), dsrc, sizeof(T) * tmp.size(), hipMemcpyDeviceToHost));
  for (int j = 0; j < nr; j++) std::memcpy(dst + (size_t)W->perm[j] * width, tmp.data() + (size_t)j * width, sizeof(T) * width);
  return SDSO_OK;
}
// the 19-float projection records (projectedTo 16, centerProjectedTo 3) into the caller's two arrays, window order; either may be NULL
static int fetch_projections(sdso_ctx* ctx, const BaWindowDev* W, const float* dsrc, float* projectedTo, float* centerProjectedTo) {
  std::vector<float> pj((size_t)W->d.nr * 19);
  const int rc = fetch_to_window_order(ctx, W, dsrc, 19, pj.data());
  if (rc) return rc;
  for (int o = 0; o < W->d.nr; o++) {
    if (projectedTo) std::memcpy(projectedTo + (size_t)o * 16, &pj[(size_t)o * 19], 64);
    if (centerProjectedTo) std::memcpy(centerProjectedTo + (size_t)o * 3, &pj[(size_t)o * 19 + 16], 12);
  }
  return SDSO_OK;
}
// xAd[nf*h+t] = xF(h)^T adHostF[h+nf*t] + xF(t)^T adTargetF[h+nf*t] from the float adjoints (EnergyFunctional.cpp:283-292), as k_ba_solve leaves it
static std::vector<float> host_xAd(const BaWindowDev* W, const double* x) {
  const int nf = W->d.nf;
  std::vector<float> xAd((size_t)nf * nf * 8);
  for (int h = 0; h < nf; h++)
    for (int t = 0; t < nf; t++)
      for (int j = 0; j < 8; j++) {
        float sh = 0, stt = 0;
        for (int i = 0; i < 8; i++) {
          sh += (float)x[4 + 8 * h + i] * (float)W->tab.adHost[(size_t)(h + nf * t) * 64 + i * 8 + j];
          stt += (float)x[4 + 8 * t + i] * (float)W->tab.adTarget[(size_t)(h + nf * t) * 64 + i * 8 + j];
        }
        xAd[(size_t)(nf * h + t) * 8 + j] = sh + stt;
      }
  return xAd;
}
// frame and calibration steps = -x (EnergyFunctional.cpp:283-286)
static void set_steps_from_x(BaWindowDev* W, const double* x) {
  for (int i = 0; i < 4; i++) W->calib.step[i] = -x[i];
  for (int f = 0; f < W->d.nf; f++) {
    for (int i = 0; i < 8; i++) W->frames[f].step[i] = -x[4 + 8 * f + i];
    W->frames[f].step[8] = W->frames[f].step[9] = 0;
  }
}
// nres[0] of the latest accumulateAF and accumulateLF from the packed accumulators (EnergyFunctional.cpp:219, :241): one blocking copy
static int read_nres(sdso_ctx* ctx, const BaWindowDev* W, int* nresA, int* nresL) {
  float nres2[2] = {0, 0};
  SDSO_HIP(ctx, hipMemcpy(nres2, W->d.accum + acc_off_nres(W->d.nf), sizeof(nres2), hipMemcpyDeviceToHost));
  if (nresA) *nresA = (int)nres2[0];
  if (nresL) *nresL = (int)nres2[1];
  return SDSO_OK;
}
// setNewFrameEnergyTH (FullSystemOptimize.cpp:98-139) from the energies the linearize kernel wrote
static int update_frame_energy_th(sdso_ctx* ctx, BaWindowDev* W) {
  const int nr = W->d.nr, nf = W->d.nf;
  std::vector<float> e(nr);
  if (nr) SDSO_HIP(ctx, hipMemcpyAsync(e.data(), W->d.r_newEnergyWO, sizeof(float) * nr, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<float> all;
  all.reserve(nr);
  for (int j = 0; j < nr; j++)
    if (!W->h_lin[j] && e[j] >= 0 && W->h_target[j] == nf - 1) all.push_back(e[j]);
  float th;
  if (all.empty()) th = 12 * 12 * 8;
  else {
    const int nth = (int)(0.7f * all.size());
    std::nth_element(all.begin(), all.begin() + nth, all.end());
    const float nthElement = sqrtf(all[nth]);
    th = nthElement * 1.5f;
    th = 26.0f * 0.5f + th * (1 - 0.5f);
    th = th * th;
    th *= 1.0f * 1.0f;
  }
  W->frames[nf - 1].frameEnergyTH = th;
  SDSO_HIP(ctx, hipMemcpyAsync(W->dt_frameTH + (nf - 1), &W->frames[nf - 1].frameEnergyTH, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

// FullSystem::linearizeAll(fixLinearization) (FullSystemOptimize.cpp:142-203)
static int linearize_all(sdso_ctx* ctx, BaWindowDev* W, bool fix, double* energy) {
  BaLaunch L = single(W);
  launch_linearize(ctx, L);
  W->j_inplace_last = false;
  if (fix) launch_apply(ctx, L);
  SDSO_HIP(ctx, hipGetLastError());
  std::vector<double> ep(W->nblk_res);
  if (W->nblk_res) SDSO_HIP(ctx, hipMemcpyAsync(ep.data(), W->d.e_part, sizeof(double) * W->nblk_res, hipMemcpyDeviceToHost, ctx->stream));
  int rc = update_frame_energy_th(ctx, W);  // synchronises
  if (rc) return rc;
  double s = 0;
  for (double v : ep) s += v;
  if (energy) *energy = s;
  W->accumulated = false;
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_ba_linearize(sdso_ctx* ctx, int win, double* energy) {
  GET_WIN();
  return linearize_all(ctx, W, false, energy);
}

namespace sdso {
// RawResidualJacobian records in the ABI's field order; ef = false: PointFrameResidual::J (= J[1 - jsel], what linearize wrote
// last — or J[jsel] when that was the fused kernel refreshing the record in place), ef = true: EFResidual::J (= J[jsel], what takeDataF swapped in)
static int fetch_jacobians(sdso_ctx* ctx, BaWindowDev* W, bool ef, float* J) {
  const int nr = W->d.nr, S = W->d.nrp;
  std::vector<float> j0((size_t)76 * S), j1((size_t)76 * S);
  std::vector<uint8_t> sel(nr);
  SDSO_HIP(ctx, hipMemcpy(j0.data(), W->d.J[0], sizeof(float) * j0.size(), hipMemcpyDeviceToHost));
  SDSO_HIP(ctx, hipMemcpy(j1.data(), W->d.J[1], sizeof(float) * j1.size(), hipMemcpyDeviceToHost));
  if (nr) SDSO_HIP(ctx, hipMemcpy(sel.data(), W->d.r_jsel, nr, hipMemcpyDeviceToHost));
  const bool both_ef = W->j_inplace_last;     // fused kernel, in place: "what linearize wrote last" sits in the EF slot too
  for (int j = 0; j < nr; j++) {
    const std::vector<float>& src = ((sel[j] != 0) != (ef || both_ef)) ? j0 : j1;
    float* o = J + (size_t)W->perm[j] * 74;
    for (int f = 0; f < 74; f++) { const int dv = jdev(f); o[f] = src[j_off(S, j, dv >> 2) + (dv & 3)]; }
  }
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_ba_get_ef_jacobians(sdso_ctx* ctx, int win, float* J) {
  GET_WIN();
  SDSO_REQUIRE(ctx, J, "null buffer");
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return fetch_jacobians(ctx, W, true, J);
}

extern "C" int sdso_ba_get_linearization(sdso_ctx* ctx, int win, float* J, uint8_t* newState, float* newEnergy, float* newEnergyWithOutlier,
                                         float* projectedTo, float* centerProjectedTo) {
  GET_WIN();
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (J) { const int rcj = fetch_jacobians(ctx, W, false, J); if (rcj) return rcj; }
  int rc = SDSO_OK;
  if (newState) rc |= fetch_to_window_order(ctx, W, W->d.r_newState, 1, newState);
  if (newEnergy) rc |= fetch_to_window_order(ctx, W, W->d.r_newEnergy, 1, newEnergy);
  if (newEnergyWithOutlier) rc |= fetch_to_window_order(ctx, W, W->d.r_newEnergyWO, 1, newEnergyWithOutlier);
  if (projectedTo || centerProjectedTo) {
    SDSO_REQUIRE(ctx, W->d.r_proj, "projections were not kept: call sdso_ba_keep_projections(ctx, win, 1) before linearize");
    rc |= fetch_projections(ctx, W, W->d.r_proj, projectedTo, centerProjectedTo);
  }
  return rc;
}

extern "C" int sdso_ba_apply_res(sdso_ctx* ctx, int win) {
  GET_WIN();
  launch_apply(ctx, single(W));
  SDSO_HIP(ctx, hipGetLastError());
  W->accumulated = false;
  return SDSO_OK;
}

extern "C" int sdso_ba_get_residual_state(sdso_ctx* ctx, int win, uint8_t* state, uint8_t* isActive, float* JpJdF) {
  GET_WIN();
  const int nr = W->d.nr;
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int rc = SDSO_OK;
  if (state && (rc = fetch_to_window_order(ctx, W, W->d.r_state, 1, state))) return rc;
  if (isActive && (rc = fetch_to_window_order(ctx, W, W->d.r_act, 1, isActive))) return rc;
  if (JpJdF && nr) {   // (the records lie in the window's order)
    std::vector<float> rec((size_t)nr * 16);
    SDSO_HIP(ctx, hipMemcpy(rec.data(), W->d.r_rec, sizeof(float) * rec.size(), hipMemcpyDeviceToHost));
    for (int o = 0; o < nr; o++) std::memcpy(JpJdF + (size_t)o * 8, &rec[(size_t)o * 16], 32);
  }
  return SDSO_OK;
}

extern "C" int sdso_ba_accumulate(sdso_ctx* ctx, int win) {
  GET_WIN();
  launch_accumulate(ctx, single(W), nullptr, false);
  SDSO_HIP(ctx, hipGetLastError());
  W->accumulated = true; W->marg_accumulated = false;
  return SDSO_OK;
}

extern "C" int sdso_ba_accum_dev(sdso_ctx* ctx, int win, void** dev_ptr) {
  GET_WIN();
  SDSO_REQUIRE(ctx, dev_ptr, "null out pointer");
  ensure_folded_win(ctx, W);
  *dev_ptr = W->d.accum;
  return SDSO_OK;
}

extern "C" int sdso_ba_get_accumulators(sdso_ctx* ctx, int win, float* packed) {
  GET_WIN();
  SDSO_REQUIRE(ctx, packed, "null buffer");
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ensure_folded_win(ctx, W);
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SDSO_HIP(ctx, hipMemcpy(packed, W->d.accum, sizeof(float) * acc_floats(W->d.nf), hipMemcpyDeviceToHost));
  return SDSO_OK;
}

// overwrite the packed accumulators (after a host-side / non-RCCL reduction across ranks)
extern "C" int sdso_ba_set_accumulators(sdso_ctx* ctx, int win, const float* packed) {
  GET_WIN();
  SDSO_REQUIRE(ctx, packed, "null buffer");
  ensure_folded_win(ctx, W);
  SDSO_HIP(ctx, hipMemcpyAsync(W->d.accum, packed, sizeof(float) * acc_floats(W->d.nf), hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  W->accumulated = true;
  return SDSO_OK;
}

extern "C" int sdso_ba_get_point_terms(sdso_ctx* ctx, int win, float* HdiF, float* bdSumF, float* Hdd_accAF, float* bd_accAF, float* Hcd_accAF) {
  GET_WIN();
  ensure_folded_win(ctx, W);      // (joins a Schur kernel that is still on the side stream)
  const int np = W->d.np;
  std::vector<float> po((size_t)np * 16);
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (np) SDSO_HIP(ctx, hipMemcpy(po.data(), W->d.p_out, sizeof(float) * po.size(), hipMemcpyDeviceToHost));
  for (int p = 0; p < np; p++) {
    const float* o = &po[(size_t)p * 16];
    if (HdiF) HdiF[p] = o[PO_HDI];
    if (bdSumF) bdSumF[p] = o[PO_BDSUM];
    if (Hdd_accAF) Hdd_accAF[p] = o[PO_HDD_A];
    if (bd_accAF) bd_accAF[p] = o[PO_BD_A];
    if (Hcd_accAF) for (int k = 0; k < 4; k++) Hcd_accAF[p * 4 + k] = o[PO_HCD_A + k];
  }
  return SDSO_OK;
}

namespace sdso {
// solveSystemF's non-default branches (EnergyFunctional.cpp:876-900 SOLVER_ORTHOGONALIZE_SYSTEM, :924-965 SOLVER_SVD [_CUT7]):
// the stitched 68x68 blocks come back from the device, the assembly and the solve run on the host in double (a Jacobi
// eigen-decomposition stands in for Eigen::JacobiSVD of the symmetric matrix), x / lastHS / lastbS go back for the
// back-substitution kernel.  Single-window path only; the batch entry points keep the default branch.
static int solve_system_host(sdso_ctx* ctx, BaWindowDev* W, int iteration, double lambda) {
  { const int rcs = sync_prior_host(ctx, W); if (rcs) return rcs; }
  const BaLaunch L = single(W);
  const int nf = L.nf, n = L.n;
  launch_stitch(ctx, L);
  SDSO_HIP(ctx, hipGetLastError());
  const size_t blk = (size_t)n * n + n;
  std::vector<double> st(3 * blk);
  SDSO_HIP(ctx, hipMemcpyAsync(st.data(), W->d.sol, sizeof(double) * st.size(), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const double *HA = st.data(), *bA = HA + (size_t)n * n, *HL = st.data() + blk, *bL = HL + (size_t)n * n, *HS = st.data() + 2 * blk, *bS = HS + (size_t)n * n;
  std::vector<double> delta(n), bM_top(n);
  for (int i = 0; i < 4; i++) delta[i] = (double)W->tab.cDeltaF[i];
  for (int f = 0; f < nf; f++) for (int i = 0; i < 8; i++) delta[4 + 8 * f + i] = W->frames[f].delta[i];
  for (int i = 0; i < n; i++) { double s = 0; for (int k = 0; k < n; k++) s += W->HM[(size_t)i * n + k] * delta[k]; bM_top[i] = W->bM[i] + s; }
  Dense Hf(n);
  std::vector<double> bf(n), lastHS((size_t)n * n), lastbS(n);
  auto orthogonalize = [&](std::vector<double>* b, Dense* H) {   // EnergyFunctional.cpp:775-835 with the window's projector
    const Dense& P = W->P;
    if (b) { std::vector<double> Pb(n, 0.0); for (int i = 0; i < n; i++) { double s = 0; for (int k = 0; k < n; k++) s += P(i, k) * (*b)[k]; Pb[i] = s; } for (int i = 0; i < n; i++) (*b)[i] -= Pb[i]; }
    if (H) {
      Dense PH(n), PHP(n);
      for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) { double s = 0; for (int k = 0; k < n; k++) s += P(i, k) * (*H)(k, j); PH(i, j) = s; }
      for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) { double s = 0; for (int k = 0; k < n; k++) s += PH(i, k) * P(k, j); PHP(i, j) = s; }
      for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) (*H)(i, j) -= PHP(i, j);
    }
  };
  if (W->solverMode & SOLVER_ORTHOGONALIZE_SYSTEM) {
    bool haveFirstFrame = false;
    for (const HostFrame& f : W->frames) if (f.frameID == 0) haveFirstFrame = true;
    Dense HT(n);
    std::vector<double> bT(n);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) HT(i, j) = HL[(size_t)i * n + j] + HA[(size_t)i * n + j] - HS[(size_t)i * n + j]; bT[i] = bL[i] + bA[i] - bS[i]; }
    if (!haveFirstFrame) orthogonalize(&bT, &HT);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) Hf(i, j) = HT(i, j) + W->HM[(size_t)i * n + j]; bf[i] = bT[i] + bM_top[i]; }
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) lastHS[(size_t)i * n + j] = Hf(i, j); lastbS[i] = bf[i]; }
    for (int i = 0; i < n; i++) Hf(i, i) *= (1 + lambda);
  } else {
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < n; j++) Hf(i, j) = HL[(size_t)i * n + j] + W->HM[(size_t)i * n + j] + HA[(size_t)i * n + j];
      bf[i] = bL[i] + bM_top[i] + bA[i] - bS[i];
    }
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) lastHS[(size_t)i * n + j] = Hf(i, j) - HS[(size_t)i * n + j]; lastbS[i] = bf[i]; }
    for (int i = 0; i < n; i++) Hf(i, i) *= (1 + lambda);
    const double f = (double)(1.0f / (1 + lambda));
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) Hf(i, j) -= HS[(size_t)i * n + j] * f;
  }
  std::vector<double> x(n, 0.0);
  if (W->solverMode & SOLVER_SVD) {
    std::vector<double> sv(n), bs(n), w;
    for (int i = 0; i < n; i++) sv[i] = 1.0 / std::sqrt(Hf(i, i));
    Dense Hs(n), V;
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) Hs(i, j) = sv[i] * Hf(i, j) * sv[j]; bs[i] = sv[i] * bf[i]; }
    symEigen(Hs, w, V);
    std::vector<int> ord(n);
    for (int i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return std::fabs(w[a]) > std::fabs(w[b]); });
    double maxSv = 0;
    for (int i = 0; i < n; i++) maxSv = std::max(maxSv, std::fabs(w[i]));
    for (int i = 0; i < n; i++) {
      const int c = ord[i];
      const double S = std::fabs(w[c]);
      double ub = 0;
      for (int k = 0; k < n; k++) ub += V(k, c) * bs[k];
      if (w[c] < 0) ub = -ub;
      if (S < kSolverModeDelta * maxSv) ub = 0;                            // setting_solverModeDelta, settings.cpp:52
      if ((W->solverMode & SOLVER_SVD_CUT7) && (i >= n - 7)) ub = 0;
      else ub /= S;
      for (int k = 0; k < n; k++) x[k] += V(k, c) * ub;
    }
    for (int k = 0; k < n; k++) x[k] *= sv[k];
  } else {
    std::vector<double> sv(n), bs(n), y;
    for (int i = 0; i < n; i++) sv[i] = 1.0 / std::sqrt(Hf(i, i) + 10);
    Dense Hs(n);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) Hs(i, j) = sv[i] * Hf(i, j) * sv[j]; bs[i] = sv[i] * bf[i]; }
    solveLdlt(Hs, bs, y);
    for (int i = 0; i < n; i++) x[i] = sv[i] * y[i];
  }
  if (solver_orth_x(W->solverMode, iteration >= 2)) orthogonalize(&x, nullptr);
  SDSO_HIP(ctx, hipMemcpyAsync(sol_x(W->d), x.data(), sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(sol_last_hs(W->d), lastHS.data(), sizeof(double) * n * n, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(sol_last_bs(W->d), lastbS.data(), sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  const std::vector<float> xAd = host_xAd(W, x.data());
  SDSO_HIP(ctx, hipMemcpyAsync(W->dt_xAd, xAd.data(), sizeof(float) * xAd.size(), hipMemcpyHostToDevice, ctx->stream));
  if (L.max_nblk_pts > 0) LAUNCH_RESUB(L, dim3(L.max_nblk_pts, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // x / lastHS / lastbS / xAd are stack-local
  return SDSO_OK;
}
static int solve_system(sdso_ctx* ctx, BaWindowDev* W, int iteration, double lambda) {
  lambda = solver_lambda(W->solverMode, lambda);
  if (solver_alt(W->solverMode) && solve_on_host()) return solve_system_host(ctx, W, iteration, lambda);
  launch_solve(ctx, single(W), lambda, solver_orth_x(W->solverMode, iteration >= 2) ? 1 : 0);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
static int fetch_x(sdso_ctx* ctx, BaWindowDev* W, std::vector<double>& x) {
  const int n = W->d.n;
  x.resize(n);
  SDSO_HIP(ctx, hipMemcpyAsync(x.data(), sol_x(W->d), sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  set_steps_from_x(W, x.data());
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_ba_solve(sdso_ctx* ctx, int win, int iteration, double lambda, double* x, double* HS, double* bS, double* frame_step, double* calib_step) {
  GET_WIN();
  SDSO_REQUIRE(ctx, W->accumulated, "sdso_ba_solve needs sdso_ba_accumulate (and, across ranks, the all-reduce of the packed accumulators) first");
  int rc = solve_system(ctx, W, iteration, lambda);
  if (rc) return rc;
  std::vector<double> xs;
  rc = fetch_x(ctx, W, xs);
  if (rc) return rc;
  const int n = W->d.n;
  if (x) std::memcpy(x, xs.data(), sizeof(double) * n);
  if (HS) SDSO_HIP(ctx, hipMemcpy(HS, sol_last_hs(W->d), sizeof(double) * n * n, hipMemcpyDeviceToHost));
  if (bS) SDSO_HIP(ctx, hipMemcpy(bS, sol_last_bs(W->d), sizeof(double) * n, hipMemcpyDeviceToHost));
  if (frame_step) for (int f = 0; f < W->d.nf; f++) for (int i = 0; i < 8; i++) frame_step[f * 8 + i] = W->frames[f].step[i];
  if (calib_step) for (int i = 0; i < 4; i++) calib_step[i] = W->calib.step[i];
  return SDSO_OK;
}

extern "C" int sdso_ba_get_stitched(sdso_ctx* ctx, int win, double* HA, double* bA, double* HL, double* bL, double* Hsc, double* bsc) {
  GET_WIN();
  SDSO_REQUIRE(ctx, W->accumulated || W->marg_accumulated, "sdso_ba_get_stitched needs sdso_ba_accumulate (or sdso_ba_marginalize_points) first");
  ensure_folded_win(ctx, W);
  launch_stitch(ctx, single(W));
  SDSO_HIP(ctx, hipGetLastError());
  const int n = W->d.n;
  const size_t blk = (size_t)n * n + n;
  std::vector<double> st(3 * blk);
  SDSO_HIP(ctx, hipMemcpyAsync(st.data(), W->d.sol, sizeof(double) * st.size(), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double* Hs[3] = {HA, HL, Hsc};
  double* bs[3] = {bA, bL, bsc};
  for (int k = 0; k < 3; k++) {
    if (Hs[k]) std::memcpy(Hs[k], st.data() + k * blk, sizeof(double) * n * n);
    if (bs[k]) std::memcpy(bs[k], st.data() + k * blk + (size_t)n * n, sizeof(double) * n);
  }
  return SDSO_OK;
}

// EnergyFunctional::resubstituteF_MT (EnergyFunctional.cpp:272-341) for a caller-supplied x: frame / calibration steps = -x, xAd from the
// float adjoints (:283-292), then resubstituteFPt for every point on the device
extern "C" int sdso_ba_resubstitute(sdso_ctx* ctx, int win, const double* x, double* frame_step, double* calib_step) {
  GET_WIN();
  SDSO_REQUIRE(ctx, x, "null x");
  SDSO_REQUIRE(ctx, W->accumulated, "sdso_ba_resubstitute needs the per-point terms of sdso_ba_accumulate");
  const int nf = W->d.nf, n = W->d.n;
  ensure_folded_win(ctx, W);
  SDSO_HIP(ctx, hipMemcpyAsync(sol_x(W->d), x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  const std::vector<float> xAd = host_xAd(W, x);
  SDSO_HIP(ctx, hipMemcpyAsync(W->dt_xAd, xAd.data(), sizeof(float) * xAd.size(), hipMemcpyHostToDevice, ctx->stream));
  const BaLaunch L = single(W);
  if (L.max_nblk_pts > 0) LAUNCH_RESUB(L, dim3(L.max_nblk_pts, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  set_steps_from_x(W, x);
  if (frame_step) for (int f = 0; f < nf; f++) for (int i = 0; i < 8; i++) frame_step[f * 8 + i] = W->frames[f].step[i];
  if (calib_step) for (int i = 0; i < 4; i++) calib_step[i] = W->calib.step[i];
  return SDSO_OK;
}

extern "C" int sdso_ba_get_point_steps(sdso_ctx* ctx, int win, float* step) {
  GET_WIN();
  const int np = W->d.np;
  std::vector<float> po((size_t)np * 16);
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (np) SDSO_HIP(ctx, hipMemcpy(po.data(), W->d.p_out, sizeof(float) * po.size(), hipMemcpyDeviceToHost));
  for (int p = 0; p < np; p++) step[p] = po[(size_t)p * 16 + PO_STEP];
  return SDSO_OK;
}

extern "C" int sdso_ba_get_tables(sdso_ctx* ctx, int win, float* precalc, double* adHost, double* adTarget, float* adHTdeltaF) {
  GET_WIN();
  const int nf = W->d.nf;
  if (precalc) std::memcpy(precalc, W->tab.precalc.data(), sizeof(float) * nf * nf * 27);
  if (adHost) std::memcpy(adHost, W->tab.adHost.data(), sizeof(double) * nf * nf * 64);
  if (adTarget) std::memcpy(adTarget, W->tab.adTarget.data(), sizeof(double) * nf * nf * 64);
  if (adHTdeltaF) std::memcpy(adHTdeltaF, W->tab.adHTdeltaF.data(), sizeof(float) * nf * nf * 8);
  return SDSO_OK;
}

// EnergyFunctional::calcLEnergyF_MT (EnergyFunctional.cpp:420-442) and calcMEnergyF (:344-351); both are 0 under
// setting_forceAceptStep (FullSystemOptimize.cpp:374-376, :1056)
static int calc_energies(sdso_ctx* ctx, BaWindowDev* W, double* EL, double* EM, bool always = false) {
  *EL = 0; *EM = 0;
  if (W->forceAccept && !always) return SDSO_OK;
  const int nf = W->d.nf, n = W->d.n;
  const int nblk = W->d.nchunks + W->nblk_pts;
  double E = 0;
  for (const HostFrame& f : W->frames) for (int i = 0; i < 8; i++) E += f.delta_prior[i] * f.prior[i] * f.delta_prior[i];
  { float s = 0; for (int i = 0; i < 4; i++) s += W->tab.cDeltaF[i] * (float)W->tab.cPrior[i] * W->tab.cDeltaF[i]; E += s; }
  if (nblk > 0) {
    int rc = ensure_scratch(ctx, sizeof(float) * nblk);
    if (rc) return rc;
    BaLaunch L = single(W);
    hipLaunchKernelGGL(k_ba_lenergy, dim3(nblk, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, (float*)ctx->scratch);
    std::vector<float> part(nblk);
    SDSO_HIP(ctx, hipMemcpyAsync(part.data(), ctx->scratch, sizeof(float) * nblk, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float Ept = 0;
    for (int b = 0; b < nblk; b++) Ept += part[b];
    E += Ept;
  }
  *EL = E;
  { const int rcs = sync_prior_host(ctx, W); if (rcs) return rcs; }
  std::vector<double> delta(n);                               // getStitchedDeltaF (:1021-1032)
  for (int i = 0; i < 4; i++) delta[i] = (double)W->tab.cDeltaF[i];       // d.head<CPARS>() = cDeltaF.cast<double>()
  for (int f = 0; f < nf; f++) for (int i = 0; i < 8; i++) delta[4 + 8 * f + i] = W->frames[f].delta[i];
  double em = 0;
  for (int i = 0; i < n; i++) { double s = 0; for (int k = 0; k < n; k++) s += W->HM[(size_t)i * n + k] * delta[k]; em += delta[i] * (2 * W->bM[i] + s); }
  *EM = em;
  return SDSO_OK;
}

// EnergyFunctional::calcLEnergyF_MT (EnergyFunctional.cpp:420-442) and calcMEnergyF (:344-351) as members a caller may invoke: the values
// themselves, whatever setting_forceAceptStep says (that test lives in FullSystem::calcLEnergy / calcMEnergy, FullSystemOptimize.cpp:374-376)
extern "C" int sdso_ba_calc_energies(sdso_ctx* ctx, int win, double* EL, double* EM) {
  GET_WIN();
  double el = 0, em = 0;
  const int rc = calc_energies(ctx, W, &el, &em, true);
  if (rc) return rc;
  if (EL) *EL = el;
  if (EM) *EM = em;
  return SDSO_OK;
}

// What EnergyFunctional::setDeltaF leaves in the reference's objects (EnergyFunctional.cpp:173-207) at the window's current state:
// cDeltaF (4 floats), EFFrame::delta / delta_prior (nf*8 doubles each), EFPoint::deltaF (np floats).  Any pointer may be NULL.
extern "C" int sdso_ba_get_deltas(sdso_ctx* ctx, int win, float* cDeltaF, double* frame_delta, double* frame_delta_prior, float* point_deltaF) {
  GET_WIN();
  const int nf = W->d.nf, np = W->d.np;
  if (cDeltaF) for (int i = 0; i < 4; i++) cDeltaF[i] = W->tab.cDeltaF[i];
  for (int f = 0; f < nf; f++)
    for (int i = 0; i < 8; i++) {
      if (frame_delta) frame_delta[f * 8 + i] = W->frames[f].delta[i];
      if (frame_delta_prior) frame_delta_prior[f * 8 + i] = W->frames[f].delta_prior[i];
    }
  if (point_deltaF && np) {
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SDSO_HIP(ctx, hipMemcpy(point_deltaF, W->d.p_delta, sizeof(float) * np, hipMemcpyDeviceToHost));
  }
  return SDSO_OK;
}

// FrameHessian::state, PointHessian::idepth and the residual states of one window as they stand (after sdso_ba_optimize /
// sdso_ba_batch_optimize); synchronises
namespace sdso {
static int get_state(sdso_ctx* ctx, BaWindowDev* W, double* state_out, float* idepth_out, uint8_t* res_state_out) {
  const int nf = W->d.nf, np = W->d.np;
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (state_out) for (int f = 0; f < nf; f++) for (int i = 0; i < 10; i++) state_out[f * 10 + i] = W->frames[f].state[i];
  if (idepth_out && np) {
    std::vector<float4> geo(np);
    SDSO_HIP(ctx, hipMemcpy(geo.data(), W->d.p_geo, sizeof(float4) * np, hipMemcpyDeviceToHost));
    for (int p = 0; p < np; p++) idepth_out[p] = geo[p].z;
  }
  if (res_state_out) return fetch_to_window_order(ctx, W, W->d.r_state, 1, res_state_out);
  return SDSO_OK;
}
}  // namespace sdso
extern "C" int sdso_ba_get_state(sdso_ctx* ctx, int win, double* state_out /* nf*10 */, float* idepth_out /* np */, uint8_t* res_state_out /* nr */) {
  GET_WIN();
  return get_state(ctx, W, state_out, idepth_out, res_state_out);
}

// Everything FullSystem::optimize leaves behind for its callers (include/sdso_abi.h: sdso_ba_post_state_t).  The per-residual part of
// linearizeAll_Reductor(true) (maxRelBaseline, numGoodResiduals; FullSystemOptimize.cpp:62-78) runs here, once per optimize call.
extern "C" int sdso_ba_get_post_state(sdso_ctx* ctx, int win, sdso_ba_post_state_t* out) {
  GET_WIN();
  SDSO_REQUIRE(ctx, out, "null post-state");
  SDSO_REQUIRE(ctx, W->post_valid, "sdso_ba_get_post_state needs a finished sdso_ba_optimize / sdso_ba_batch_optimize on this window");
  SDSO_REQUIRE(ctx, (!out->lastHS && !out->lastbS) || W->hs_valid, "lastHS / lastbS were not kept: sdso_ba_batch_keep_system(ctx, 1) before the batch loop");
  const int nf = W->d.nf, np = W->d.np, nr = W->d.nr, n = W->d.n;
  if (nr && (out->centerProjectedTo || out->projectedTo)) {
    // (the projections are re-evaluated on every call that asks for them; the counters moved when the optimize call ended)
    if (!W->d_post) { DM(W->d_post, float, (size_t)std::max(nr, 1) * 19); }
    hipLaunchKernelGGL(k_ba_post_state, dim3(std::max(W->nblk_res, 1), 1), dim3(BA_BLOCK), 0, ctx->stream, (const BaDev*)W->d_self, W->d_post, 0);
    SDSO_HIP(ctx, hipGetLastError());
  }
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // ---- points
  if (np && (out->idepth || out->step || out->HdiF || out->bdSumF || out->idepth_hessian || out->maxRelBaseline || out->numGoodResiduals)) {
    std::vector<float4> geo(np), tr(np);
    std::vector<float> po((size_t)np * 16);
    SDSO_HIP(ctx, hipMemcpy(geo.data(), W->d.p_geo, sizeof(float4) * np, hipMemcpyDeviceToHost));
    SDSO_HIP(ctx, hipMemcpy(tr.data(), W->d.p_track, sizeof(float4) * np, hipMemcpyDeviceToHost));
    SDSO_HIP(ctx, hipMemcpy(po.data(), W->d.p_out, sizeof(float) * po.size(), hipMemcpyDeviceToHost));
    for (int p = 0; p < np; p++) {
      const float* o = &po[(size_t)p * 16];
      if (out->idepth) out->idepth[p] = geo[p].z;
      if (out->step) out->step[p] = o[PO_STEP];
      if (out->HdiF) out->HdiF[p] = o[PO_HDI];
      if (out->bdSumF) out->bdSumF[p] = o[PO_BDSUM];
      if (out->idepth_hessian) out->idepth_hessian[p] = tr[p].z;
      if (out->maxRelBaseline) out->maxRelBaseline[p] = tr[p].x;
      if (out->numGoodResiduals) std::memcpy(&out->numGoodResiduals[p], &tr[p].y, 4);
    }
  }
  // ---- residuals (pair-sorted on the device -> the window's order)
  out->n_toRemove = 0;
  if (nr) {
    std::vector<uint8_t> st(nr), act(nr), lin(nr);
    int rc;
    if ((rc = fetch_to_window_order(ctx, W, W->d.r_state, 1, st.data()))) return rc;
    if ((rc = fetch_to_window_order(ctx, W, W->d.r_act, 1, act.data()))) return rc;
    if ((rc = fetch_to_window_order(ctx, W, W->d.r_lin, 1, lin.data()))) return rc;
    for (int o = 0; o < nr; o++) {
      const bool rem = !(lin[o] & 1) && !act[o];      // in activeResiduals and not isActive(): toRemove (:80-84)
      if (out->state_state) out->state_state[o] = st[o];
      if (out->isActiveAndIsGoodNEW) out->isActiveAndIsGoodNEW[o] = act[o];
      if (out->toRemove) out->toRemove[o] = rem ? 1 : 0;
      out->n_toRemove += rem ? 1 : 0;
    }
    if (out->state_energy && (rc = fetch_to_window_order(ctx, W, W->d.r_energy, 1, out->state_energy))) return rc;
    if ((out->centerProjectedTo || out->projectedTo) && (rc = fetch_projections(ctx, W, W->d_post, out->projectedTo, out->centerProjectedTo))) return rc;
  }
  // ---- frames, calibration (host mirror: brought up to date when the loop ended)
  std::vector<double> x(n);
  SDSO_HIP(ctx, hipMemcpy(x.data(), sol_x(W->d), sizeof(double) * n, hipMemcpyDeviceToHost));
  for (int f = 0; f < nf; f++) {
    const HostFrame& F = W->frames[f];
    for (int i = 0; i < 10; i++) {
      if (out->state) out->state[f * 10 + i] = F.state[i];
      if (out->state_zero) out->state_zero[f * 10 + i] = F.state_zero[i];
      if (out->frame_step) out->frame_step[f * 10 + i] = i < 8 ? -x[4 + 8 * f + i] : 0.0;   // EnergyFunctional.cpp:283-286
    }
    if (out->evalPT) { std::memcpy(out->evalPT + f * 12, F.evalPT.R.data(), 72); std::memcpy(out->evalPT + f * 12 + 9, F.evalPT.t.data(), 24); }
    if (out->PRE_worldToCam) { std::memcpy(out->PRE_worldToCam + f * 12, F.PRE_worldToCam.R.data(), 72); std::memcpy(out->PRE_worldToCam + f * 12 + 9, F.PRE_worldToCam.t.data(), 24); }
    if (out->frameEnergyTH) out->frameEnergyTH[f] = F.frameEnergyTH;
  }
  for (int i = 0; i < 4; i++) { out->calib_value[i] = W->calib.value[i]; out->calib_value_scaled[i] = W->calib.value_scaled[i]; out->calib_step[i] = -x[i]; }
  if (out->lastX) std::memcpy(out->lastX, x.data(), sizeof(double) * n);
  if (out->lastHS) SDSO_HIP(ctx, hipMemcpy(out->lastHS, sol_last_hs(W->d), sizeof(double) * n * n, hipMemcpyDeviceToHost));
  if (out->lastbS) SDSO_HIP(ctx, hipMemcpy(out->lastbS, sol_last_bs(W->d), sizeof(double) * n, hipMemcpyDeviceToHost));
  // (resInL: nres[0] of the last accumulateLF, EnergyFunctional.cpp:241 — recorded when the optimize call ended, next to resInA)
  out->resInA = W->last_result.resInA; out->resInL = W->resInL; out->resInM = W->resInM;
  out->result = W->last_result;
  return SDSO_OK;
}

// EnergyFunctional::resInA / resInL (nres[0] of the latest accumulateAF / LF, EnergyFunctional.cpp:219, :241) and resInM (residuals
// marginalised through this window so far, :704).  Any pointer may be NULL.
extern "C" int sdso_ba_get_counts(sdso_ctx* ctx, int win, int* resInA, int* resInL, int* resInM) {
  GET_WIN();
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (resInA || resInL) {
    ensure_folded_win(ctx, W);
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = read_nres(ctx, W, resInA, resInL);
    if (rc) return rc;
  }
  if (resInM) *resInM = W->resInM;
  return SDSO_OK;
}


// The window as sdso_track_make_ref_from_window reads it (sdso_internal.h): its device descriptor after a finished optimize call.
namespace sdso {
int ba_ref_view(sdso_ctx* ctx, int win, BaRefView* out) {
  BaWindowDev* W = find_win(ctx, win);
  if (!W) return sdso::fail(ctx, SDSO_ERR_ARG, "unknown window");
  if (!W->post_valid) return sdso::fail(ctx, SDSO_ERR_STATE, "the window has no post-state: sdso_ba_optimize first (sdso_ba_window_update discards it)");
  if (W->in_batch) return sdso::fail(ctx, SDSO_ERR_STATE, "the window is a member of a batch");
  if (W->has_lin_cached) return sdso::fail(ctx, SDSO_ERR_STATE, "the window holds a linearised residual");
  out->dev = W->d_self;
  out->nf = W->d.nf; out->np = W->d.np; out->nr = W->d.nr; out->w = W->d.w; out->h = W->d.h;
  out->last_frame_slot = W->frames[W->d.nf - 1].frame_slot;
  out->K[0] = W->d.fxl; out->K[1] = W->d.fyl; out->K[2] = W->d.cxl; out->K[3] = W->d.cyl;
  return SDSO_OK;
}
int ba_window_hosts(sdso_ctx* ctx, int win, int frameID[8], int host_pt_beg[9]) {
  BaWindowDev* W = find_win(ctx, win);
  if (!W) return sdso::fail(ctx, SDSO_ERR_ARG, "unknown window");
  for (int f = 0; f < 8; f++) frameID[f] = f < W->d.nf ? W->frames[f].frameID : -1;
  std::memcpy(host_pt_beg, W->d.host_pt_beg, sizeof(W->d.host_pt_beg));
  return SDSO_OK;
}
int ba_window_points(sdso_ctx* ctx, int win, BaPointsView* out) {
  BaWindowDev* W = find_win(ctx, win);
  if (!W) return sdso::fail(ctx, SDSO_ERR_ARG, "unknown window");
  out->p_geo = W->d.p_geo; out->p_host = W->d.p_host;
  out->nf = W->d.nf; out->np = W->d.np; out->w = W->d.w; out->h = W->d.h;
  return SDSO_OK;
}
}  // namespace sdso

