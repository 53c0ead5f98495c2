// BA host API, part 4 (included by ba.hip): marginalisation.  The points' (marginalizePointsF) and the frame's (marginalizeFrame: host
// algebra, and on the device-resident prior), and the next window's adoption of that prior.
// flagPointsForRemoval core (FullSystem.cpp:1004-1021) + EnergyFunctional::marginalizePointsF (:663-736)
extern "C" int sdso_ba_marginalize_points(sdso_ctx* ctx, int win, const uint8_t* marg_flag, double* HM_out, double* bM_out) {
  GET_WIN();
  SDSO_REQUIRE(ctx, marg_flag, "null flags");
  const int np = W->d.np, nr = W->d.nr, n = W->d.n;
  BaLaunch L = single(W);
  H2D(W->d_pflag, marg_flag, np);
  hipLaunchKernelGGL(k_ba_reset_flagged, dim3(L.max_nblk_res, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, W->d_pflag);
  hipLaunchKernelGGL(k_ba_linearize, dim3(L.max_nblk_res, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
  W->j_inplace_last = false;
  launch_apply(ctx, L);
  hipLaunchKernelGGL(k_ba_unmask, dim3(L.max_nblk_res, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
  hipLaunchKernelGGL(k_ba_fixlin, dim3(L.max_nblk_res, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, W->d_pflag);
  for (int p = 0; p < np; p++) if (marg_flag[p]) W->h_prior[p] *= 600.f * 600.f;   // setting_idepthFixPriorMargFac (:674)
  H2D(W->d.p_prior, W->h_prior.data(), sizeof(float) * np);
  launch_accumulate(ctx, L, W->d_pflag, true);
  launch_stitch(ctx, L);
  SDSO_HIP(ctx, hipGetLastError());
  // HM += setting_margWeightFac * (M - Msc), bM likewise (:727-728): on the device copy, which is the master — the prior stays resident
  // from here through sdso_ba_marginalize_frame_dev into the next window (sdso_ba_adopt_prior); the host mirror follows on demand
  if (W->solverMode & (SOLVER_ORTHOGONALIZE_POINTMARG | SOLVER_ORTHOGONALIZE_FULL))     // (:707-731; POINTMARG only when frame 0 has left the window)
    hipLaunchKernelGGL(k_ba_prior_orth, dim3(1, 1), dim3(256), 0, ctx->stream, L.d_arr, (double)(0.5f * 0.5f),
                       ((W->solverMode & SOLVER_ORTHOGONALIZE_POINTMARG) && !W->d.have_first_frame) ? 1 : 0, (W->solverMode & SOLVER_ORTHOGONALIZE_FULL) ? 1 : 0);
  else
  hipLaunchKernelGGL(k_ba_prior_add, dim3(8, 1), dim3(256), 0, ctx->stream, L.d_arr, (double)(0.5f * 0.5f));   // setting_margWeightFac
  SDSO_HIP(ctx, hipGetLastError());
  W->hm_host_valid = false;
  W->prior_pristine = false;
  W->marg_chain = false;            // the resident prior changed: the next marginalizeFrame starts from it again
  std::vector<uint8_t> lin(nr);
  if (nr) SDSO_HIP(ctx, hipMemcpyAsync(lin.data(), W->d.r_lin, nr, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  W->h_lin = lin;
  W->has_lin_cached = std::any_of(lin.begin(), lin.end(), [](uint8_t v) { return v != 0; });
  {  // resInM += accSSE_top_A->nres[0] (EnergyFunctional.cpp:704)
    int nresM = 0;
    const int rcn = read_nres(ctx, W, &nresM, nullptr);
    if (rcn) return rcn;
    W->resInM += nresM;
  }
  if (HM_out || bM_out) {
    const int rcs = sync_prior_host(ctx, W);
    if (rcs) return rcs;
    if (HM_out) std::memcpy(HM_out, W->HM.data(), sizeof(double) * n * n);
    if (bM_out) std::memcpy(bM_out, W->bM.data(), sizeof(double) * n);
  }
  W->accumulated = false;
  W->marg_accumulated = true;
  return SDSO_OK;
}

// EnergyFunctional::marginalizeFrame (EnergyFunctional.cpp:554-660): drop frame `idx` from the marginalisation prior
// HM / bM by a scaled Schur complement.  ~70x70 doubles once per keyframe: host algebra, no device work.
extern "C" int sdso_ba_marginalize_frame(int nf, int idx, const double* prior8, const double* delta_prior8, const double* HM_in,
                                         const double* bM_in, double* HM_out, double* bM_out) {
  if (nf < 1 || idx < 0 || idx >= nf || !prior8 || !delta_prior8 || !HM_in || !bM_in || !HM_out || !bM_out) return SDSO_ERR_ARG;
  const int odim = nf * 8 + 4, ndim = odim - 8;
  // step 1: move the frame's 8 rows / columns to the end (order of the others unchanged)
  std::vector<int> ord;
  for (int i = 0; i < odim; i++) if (i < idx * 8 + 4 || i >= idx * 8 + 12) ord.push_back(i);
  for (int i = 0; i < 8; i++) ord.push_back(idx * 8 + 4 + i);
  std::vector<double> H((size_t)odim * odim), b(odim);
  for (int i = 0; i < odim; i++) { b[i] = bM_in[ord[i]]; for (int j = 0; j < odim; j++) H[(size_t)i * odim + j] = HM_in[(size_t)ord[i] * odim + ord[j]]; }
  // step 2: the frame's prior
  for (int i = 0; i < 8; i++) { H[(size_t)(ndim + i) * odim + ndim + i] += prior8[i]; b[ndim + i] += prior8[i] * delta_prior8[i]; }
  // step 3: scale, invert the 8x8 corner, Schur complement, unscale
  std::vector<double> S(odim), Si(odim);
  for (int i = 0; i < odim; i++) { S[i] = std::sqrt(std::fabs(H[(size_t)i * odim + i]) + 10); Si[i] = 1.0 / S[i]; }
  for (int i = 0; i < odim; i++) { b[i] = Si[i] * b[i]; for (int j = 0; j < odim; j++) H[(size_t)i * odim + j] = Si[i] * H[(size_t)i * odim + j] * Si[j]; }
  double A[8][8], inv[8][8];
  for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) { const double v = H[(size_t)(ndim + i) * odim + ndim + j]; A[i][j] = 0.5f * (v + v); inv[i][j] = i == j; }
  for (int k = 0; k < 8; k++) {   // Gauss-Jordan, partial pivoting (Eigen's fixed-size inverse() is PartialPivLU)
    int pv = k;
    for (int i = k + 1; i < 8; i++) if (std::fabs(A[i][k]) > std::fabs(A[pv][k])) pv = i;
    if (pv != k) for (int j = 0; j < 8; j++) { std::swap(A[k][j], A[pv][j]); std::swap(inv[k][j], inv[pv][j]); }
    const double d = A[k][k];
    for (int j = 0; j < 8; j++) { A[k][j] /= d; inv[k][j] /= d; }
    for (int i = 0; i < 8; i++) {
      if (i == k) continue;
      const double f = A[i][k];
      if (f == 0) continue;
      for (int j = 0; j < 8; j++) { A[i][j] -= f * A[k][j]; inv[i][j] -= f * inv[k][j]; }
    }
  }
  for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) inv[i][j] = 0.5f * (inv[i][j] + inv[i][j]);
  std::vector<double> bli((size_t)ndim * 8);   // bottomLeft^T * hpi
  for (int r = 0; r < ndim; r++)
    for (int c = 0; c < 8; c++) { double s = 0; for (int k = 0; k < 8; k++) s += H[(size_t)(ndim + k) * odim + r] * inv[k][c]; bli[(size_t)r * 8 + c] = s; }
  for (int r = 0; r < ndim; r++) {
    for (int c = 0; c < ndim; c++) { double s = 0; for (int k = 0; k < 8; k++) s += bli[(size_t)r * 8 + k] * H[(size_t)(ndim + k) * odim + c]; H[(size_t)r * odim + c] -= s; }
    double s = 0;
    for (int k = 0; k < 8; k++) s += bli[(size_t)r * 8 + k] * b[ndim + k];
    b[r] -= s;
  }
  for (int i = 0; i < odim; i++) { b[i] = S[i] * b[i]; for (int j = 0; j < odim; j++) H[(size_t)i * odim + j] = S[i] * H[(size_t)i * odim + j] * S[j]; }
  for (int r = 0; r < ndim; r++) { bM_out[r] = b[r]; for (int c = 0; c < ndim; c++) HM_out[(size_t)r * ndim + c] = 0.5 * (H[(size_t)r * odim + c] + H[(size_t)c * odim + r]); }
  return SDSO_OK;
}

// EnergyFunctional::marginalizeFrame (EnergyFunctional.cpp:554-660) on the window's DEVICE-resident prior (k_ba_marg_frame): what
// sdso_ba_marginalize_points left in dt_HM / dt_bM goes through the frame's marginalisation without visiting the host; the result stays in
// the window (BaWindowDev::d_marg) until the next window adopts it (sdso_ba_adopt_prior).  prior / delta_prior are the frame's own
// (EFFrame::prior, delta_prior = the host mirror's, as uploaded / as the resident loop left them).  HM_out / bM_out: optional copies.
extern "C" int sdso_ba_marginalize_frame_dev(sdso_ctx* ctx, int win, int idx, double* HM_out, double* bM_out) {
  GET_WIN();
  const int nf = W->d.nf, n = W->d.n;
  // Several frames may leave at one keyframe (FullSystem.cpp:1470-1476 calls marginalizeFrame for every flagged frame, each on the prior
  // the previous one left): a call that follows another one — with no sdso_ba_marginalize_points in between — continues from that result,
  // and `idx` then counts the frames the prior still covers, as the reference's frames[] does after the earlier frame was erased.
  if (!W->marg_chain) { W->marg_frames.resize(nf); std::iota(W->marg_frames.begin(), W->marg_frames.end(), 0); }
  const int cur = (int)W->marg_frames.size(), odim = 8 * cur + 4, m = odim - 8;
  SDSO_REQUIRE(ctx, idx >= 0 && idx < cur, "frame index out of range (it counts the frames the prior still covers)");
  const size_t half = (size_t)n * n + n;
  if (!W->d_marg) { DM(W->d_marg, double, 2 * half); W->d_marg2 = W->d_marg + half; }   // ONE allocation: never d_marg without d_marg2
  const HostFrame& Fm = W->frames[W->marg_frames[idx]];
  double pr[16];
  for (int i = 0; i < 8; i++) { pr[i] = Fm.prior[i]; pr[8 + i] = Fm.delta_prior[i]; }
  int rc = ensure_scratch(ctx, sizeof(pr));
  if (rc) return rc;
  SDSO_HIP(ctx, hipMemcpyAsync(ctx->scratch, pr, sizeof(pr), hipMemcpyHostToDevice, ctx->stream));
  const double* srcH = W->marg_chain ? W->d_marg : W->dt_HM;
  const double* srcb = W->marg_chain ? W->d_marg + (size_t)odim * odim : W->dt_bM;
  hipLaunchKernelGGL(k_ba_marg_frame, dim3(1), dim3(256), 0, ctx->stream, srcH, srcb, odim, idx, (const double*)ctx->scratch, W->d_marg2);
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (pr is stack-local)
  std::swap(W->d_marg, W->d_marg2);                      // the chain advances only once the launch and the synchronisation succeeded
  W->marg_frames.erase(W->marg_frames.begin() + idx);
  W->marg_chain = true;
  W->marg_dim = m;
  if (HM_out) SDSO_HIP(ctx, hipMemcpy(HM_out, W->d_marg, sizeof(double) * m * m, hipMemcpyDeviceToHost));
  if (bM_out) SDSO_HIP(ctx, hipMemcpy(bM_out, W->d_marg + (size_t)m * m, sizeof(double) * m, hipMemcpyDeviceToHost));
  return SDSO_OK;
}

// The next window takes over the prior sdso_ba_marginalize_frame_dev left in `from_win`: device to device, the new keyframe's 8 rows /
// columns zero — what EnergyFunctional::insertFrame does to HM / bM (EnergyFunctional.cpp:468-476: conservativeResize + setZero of the new
// rows and columns).  `win` must have been uploaded with HM = bM = NULL (zeros) and its LEADING frames must be the frames the prior covers,
// in the same order (checked by frameID): a prior attached to other frames is an error, never a silent result.  (k_ba_prior_adopt: ba_solve.hip)
extern "C" int sdso_ba_adopt_prior(sdso_ctx* ctx, int win, int from_win) {
  GET_WIN();
  BaWindowDev* F = find_win(ctx, from_win);
  SDSO_REQUIRE(ctx, F && F->d_marg && F->marg_dim > 0, "the source window holds no marginalised prior (sdso_ba_marginalize_frame_dev first)");
  SDSO_REQUIRE(ctx, F != W, "a window cannot adopt its own prior");
  const int n = W->d.n, m = F->marg_dim, k = (int)F->marg_frames.size();
  SDSO_REQUIRE(ctx, m == 8 * k + 4 && m <= n, "the prior covers more frames than the window holds");
  SDSO_REQUIRE(ctx, W->prior_pristine, "the adopting window must have been uploaded with HM = bM = NULL and not have changed its prior since");
  for (int i = 0; i < k; i++)
    SDSO_REQUIRE(ctx, W->frames[i].frameID == F->frames[F->marg_frames[i]].frameID, "the window's leading frames are not the frames the prior covers (frameID mismatch)");
  hipLaunchKernelGGL(k_ba_prior_adopt, dim3(8), dim3(256), 0, ctx->stream, W->dt_HM, W->dt_bM, n, (const double*)F->d_marg, (const double*)F->d_marg + (size_t)m * m, m);
  SDSO_HIP(ctx, hipGetLastError());
  W->hm_host_valid = false;
  W->accumulated = false;
  W->prior_pristine = false;
  W->marg_chain = false;
  return SDSO_OK;
}

