// BA host API, part 6 (included by ba.hip): FullSystem::optimize.  The device-resident Gauss-Newton loop (ba_opt.hip / ba_tail.hip) over
// one window or a batch, and the host-driven loop of sdso_ba_optimize (SDSO_BA_HOST_LOOP / SDSO_BA_SOLVE_HOST, A/B).
namespace sdso {
int comm_nranks(sdso_ctx* ctx);                                                            // comm.hip
int comm_rank(sdso_ctx* ctx);                                                              // comm.hip
bool comm_present(sdso_ctx* ctx);                                                          // comm.hip
int comm_allgather_floats(sdso_ctx* ctx, const float* send, float* recv, size_t nfloats);  // comm.hip
int comm_max_int(sdso_ctx* ctx, int* value);                                               // comm.hip


// one resident loop on a ctx: a batch (sdso_ba_batch_optimize*) or a single window (sdso_ba_optimize)
struct OptRun {
  BaLaunch L{};
  std::vector<BaWindowDev*> W;
  bool materialize = true;
  int cap = 0, nranks = 1, sums_stride = 0, iteration = 0, stop = 1;
  bool exchange = false;   // pack + all-gather between the ranks (always when nranks > 1)
  bool gated = false;      // energy-gated flow (setting_forceAceptStep = false): un-fused kernels + k_ba_opt_gate
  int lstride = 0;         // floats between the windows' calcLEnergy partials
  bool active = false;
  bool local_only = false; // single-window call: never a collective, whatever communicator the ctx carries
  bool failed = false;     // a collective of the gated flow failed (sdso_last_error says which)
  bool keep_hs = false;    // every solve also writes lastHS / lastbS (EnergyFunctional.cpp:909-910): sdso_ba_get_post_state hands them out
  bool scatter_local = false;  // this rank's view: the batch asks for the reduce-scatter exchange and its loop can take it
  bool scatter = false;    // ... and every rank agreed (opt_begin)
  int momentum = 0;        // SOLVER_STEPMOMENTUM / SOLVER_MOMENTUM bits of the windows: k_ba_opt_momentum between solve and step, never the fused step
  OptBufs* B = nullptr;
};

static int opt_begin(sdso_ctx* ctx, OptRun& R, int stop_on_convergence) {
  const int nwin = (int)R.W.size(), nf = R.L.nf;
  SDSO_REQUIRE(ctx, nf >= 2, "the Gauss-Newton loop needs at least two keyframes (FullSystemOptimize.cpp:873)");
  int cap = 1;
  for (BaWindowDev* W : R.W) {
    SDSO_REQUIRE(ctx, (W->forceAccept != 0) == (R.W[0]->forceAccept != 0), "the windows of a resident loop must share setting_forceAceptStep");
    SDSO_REQUIRE(ctx, solver_branch(W->solverMode) == solver_branch(R.W[0]->solverMode), "the windows of a resident loop must share the solver branch");
    SDSO_REQUIRE(ctx, (W->solverMode & (SOLVER_MOMENTUM | SOLVER_STEPMOMENTUM)) == (R.W[0]->solverMode & (SOLVER_MOMENTUM | SOLVER_STEPMOMENTUM)), "the windows of a resident loop must share SOLVER_MOMENTUM / SOLVER_STEPMOMENTUM");
    cap = std::max(cap, W->d.nr - W->newest_first);
  }
  R.momentum = R.W[0]->solverMode & (SOLVER_MOMENTUM | SOLVER_STEPMOMENTUM);
  R.nranks = comm_nranks(ctx);
  // SDSO_OPT_FORCE_EXCHANGE: take the pack / all-gather path on a 1-rank communicator too (tests: the collectives of a 1-GPU box)
  R.exchange = !R.local_only && (R.nranks > 1 || (comm_present(ctx) && dbg_env("SDSO_OPT_FORCE_EXCHANGE") != nullptr));
  R.gated = !R.W[0]->forceAccept;
  if (R.exchange) { int rc = comm_max_int(ctx, &cap); if (rc) return rc; }
  R.cap = cap;
  // shape of the accumulators' exchange: one decision for the whole loop, the same on every rank or an error (never mismatched collectives)
  R.scatter = false;
  if (R.exchange) {
    const int want = (R.scatter_local && !R.gated && !R.keep_hs && tail_enabled() && !R.L.alt && !R.momentum && nwin % R.nranks == 0) ? 1 : 0;
    int hi = want, lo = -want;
    int rc = comm_max_int(ctx, &hi); if (rc) return rc;
    rc = comm_max_int(ctx, &lo); if (rc) return rc;
    SDSO_REQUIRE(ctx, hi == -lo, "the ranks disagree on the shape of the accumulators' exchange (sdso_ba_batch_exchange_mode / sdso_ba_batch_keep_system / SDSO_BA_TAIL differ between ranks)");
    R.scatter = want != 0;
  }
  R.sums_stride = 2 * (R.L.max_nblk_pts + 1);
  OptBufs* B = R.B = &ba_state(ctx).bufs;
  const size_t pf = opt_pack_floats(cap);
  const size_t n_sums = (size_t)nwin * R.sums_stride, n_pack = (size_t)nwin * pf, n_gather = (size_t)R.nranks * n_pack;
  SDSO_HIP(ctx, B->d_sums.reserve(ctx->stream, n_sums, n_sums));
  SDSO_HIP(ctx, B->d_pack.reserve(ctx->stream, n_pack, n_pack));
  if (R.exchange) SDSO_HIP(ctx, B->d_gather.reserve(ctx->stream, n_gather, n_gather));
  R.lstride = R.L.max_chunks + R.L.max_nblk_pts + 1;
  if (R.gated) SDSO_HIP(ctx, B->d_lpart.reserve(ctx->stream, (size_t)nwin * R.lstride, (size_t)nwin * R.lstride));
  if ((size_t)nwin > B->out_cap) {
    B->out_cap = 0;
    SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, B->d_out, B->h_out));
    SDSO_HIP(ctx, B->d_out.reserve(ctx->stream, nwin, nwin));
    SDSO_HIP(ctx, B->h_out.reserve(ctx->stream, nwin, nwin));
    B->out_cap = nwin;
  }
  for (BaWindowDev* W : R.W) {
    BaOptDev& O = W->h_opt;
    std::memset(&O, 0, sizeof(O));
    for (int f = 0; f < nf; f++) {
      const HostFrame& F = W->frames[f];
      for (int i = 0; i < 10; i++) { O.state[f][i] = F.state[i]; O.state_backup[f][i] = F.state[i]; O.state_zero[f][i] = F.state_zero[i]; }
      for (int i = 0; i < 9; i++) O.evalPT[f][i] = F.evalPT.R[i];
      for (int i = 0; i < 3; i++) O.evalPT[f][9 + i] = F.evalPT.t[i];
      O.ab_exposure[f] = F.ab_exposure;
    }
    for (int i = 0; i < 4; i++) { O.calib_value[i] = W->calib.value[i]; O.calib_backup[i] = W->calib.value[i]; O.calib_zero[i] = W->calib.value_zero[i]; }
    O.newest_first = W->newest_first;
    O.lambda = 1e-1;
    O.stepsize = 1;                                                               // FullSystemOptimize.cpp:928
    for (double& v : O.previousX) v = std::numeric_limits<double>::quiet_NaN();   // :929
    H2D(W->d_opt, &W->h_opt, sizeof(BaOptDev));
  }
  hipLaunchKernelGGL(k_ba_reset_all, dim3(R.L.max_nblk_res, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr);
  SDSO_HIP(ctx, hipGetLastError());
  R.iteration = 0; R.stop = stop_on_convergence; R.active = true;
  return SDSO_OK;
}

// pack -> [all-gather] -> k_ba_opt_step.  unfused: the energies come from k_ba_linearize's workgroups, not from the fused kernel's chunks
static int opt_consume(sdso_ctx* ctx, OptRun& R, int last, bool unfused, bool with_sums) {
  const int nwin = (int)R.W.size();
  OptBufs* B = R.B;
  const float* gathered = nullptr;     // single rank: k_ba_opt_step reads the energies where the kernels left them
  const float* sums = with_sums ? B->d_sums : (const float*)nullptr;
  if (R.exchange) {
    hipLaunchKernelGGL(k_ba_opt_pack, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, B->d_pack, R.cap, unfused ? 1 : 0, sums, R.sums_stride);
    int rc = comm_allgather_floats(ctx, B->d_pack, B->d_gather, (size_t)nwin * opt_pack_floats(R.cap));
    if (rc) return rc;
    gathered = B->d_gather;
  }
  hipLaunchKernelGGL(k_ba_opt_step, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, gathered, R.nranks, R.cap, R.iteration, last, R.stop, 1.0f, unfused ? 1 : 0, sums, R.sums_stride);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}

// after the solve of one iteration: doStepFromBackup for points, frames and calibration, tables, break test
static int opt_step(sdso_ctx* ctx, OptRun& R) {
  const int nwin = (int)R.W.size();
  if (R.momentum) hipLaunchKernelGGL(k_ba_opt_momentum, dim3(1, nwin), dim3(128), 0, ctx->stream, R.L.d_arr);   // the stepsize / the kept previous step of this iteration
  if (R.L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, dim3(R.L.max_nblk_pts, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr, 3, R.momentum ? -1.0f : 1.0f, R.B->d_sums, R.sums_stride);
  int rc = opt_consume(ctx, R, 0, false, R.L.max_nblk_pts > 0);
  R.iteration++;
  return rc;
}

// ---- energy-gated flow (setting_forceAceptStep = false): the un-fused kernels, with the decision taken by k_ba_opt_gate on the device and
// the kernels of the two branches (applyRes / loadSateBackup + re-linearisation) launched unconditionally, each looking at the decision
static void gated_linearize(sdso_ctx* ctx, OptRun& R, int cond, int which) {
  const int nwin = (int)R.W.size();
  const dim3 g(R.L.max_nblk_res, nwin), b(BA_BLOCK);
  hipLaunchKernelGGL(k_ba_linearize, g, b, 0, ctx->stream, R.L.d_arr, cond);
  mark_linearized(R.W, false);
  const int nblk = R.L.max_chunks + R.L.max_nblk_pts;
  if (nblk > 0) hipLaunchKernelGGL(k_ba_lenergy, dim3(nblk, nwin), b, 0, ctx->stream, R.L.d_arr, R.B->d_lpart, R.lstride, cond);
  if (R.exchange) {
    // sharded windows: every rank hands over its newest-frame energies, the energy of its residuals and its part of calcLEnergy; the
    // gate reads the gathered records rank by rank, so all ranks accept / reject together.  (Unconditional on every rank: a collective.)
    hipLaunchKernelGGL(k_ba_opt_pack, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, R.B->d_pack, R.cap, 1, (const float*)nullptr, 0,
                       nblk > 0 ? (const float*)R.B->d_lpart : (const float*)nullptr, R.lstride);
    if (comm_allgather_floats(ctx, R.B->d_pack, R.B->d_gather, (size_t)nwin * opt_pack_floats(R.cap))) { R.failed = true; return; }
    hipLaunchKernelGGL(k_ba_opt_gate, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, (const float*)R.B->d_lpart, R.lstride, which, R.stop,
                       (const float*)R.B->d_gather, R.nranks, R.cap);
    return;
  }
  hipLaunchKernelGGL(k_ba_opt_gate, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, (const float*)R.B->d_lpart, R.lstride, which, R.stop);
}
static int opt_gated_start(sdso_ctx* ctx, OptRun& R) {   // linearizeAll(false) + the energies of the uploaded state + applyRes (:894-908)
  const int nwin = (int)R.W.size();
  gated_linearize(ctx, R, 0, 0);
  if (R.failed) return SDSO_ERR_STATE;
  hipLaunchKernelGGL(k_ba_apply, dim3(R.L.max_nblk_res, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr, 0);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
static int opt_gated_iteration(sdso_ctx* ctx, OptRun& R, int it) {
  const int nwin = (int)R.W.size();
  const dim3 gp(std::max(R.L.max_nblk_pts, 1), nwin), b(BA_BLOCK);
  if (R.L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, gp, b, 0, ctx->stream, R.L.d_arr, 0, 0.f, (float*)nullptr, 0, 0);   // backupState
  launch_accumulate(ctx, R.L, nullptr, false);
  if (R.exchange) {                                            // sharded windows: the packed accumulators of every rank, summed
    const int rc = sdso_ba_allreduce(ctx);
    if (rc) return rc;
  }
  const int sm = R.W[0]->solverMode;
  int flags = solver_orth_x(sm, it >= 2) ? 1 : 0;
  if (solver_own_lambda(sm)) flags |= 2;                       // the loop's own lambda, kept on the device (it depends on the decisions)
  launch_solve(ctx, R.L, solver_lambda(sm, 0), flags);
  if (R.momentum) hipLaunchKernelGGL(k_ba_opt_momentum, dim3(1, nwin), dim3(128), 0, ctx->stream, R.L.d_arr);
  if (R.L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, gp, b, 0, ctx->stream, R.L.d_arr, 1, R.momentum ? -1.0f : 1.0f, R.B->d_sums, R.sums_stride, 0);
  if (R.exchange) {                                            // the break-test sums of every rank's points: pack -> all-gather -> step
    const int rc = opt_consume(ctx, R, 2, true, R.L.max_nblk_pts > 0);
    if (rc) return rc;
  } else
    hipLaunchKernelGGL(k_ba_opt_step, dim3(1, nwin), dim3(256), 0, ctx->stream, R.L.d_arr, (const float*)nullptr, 1, R.cap, it, 2, R.stop, 1.0f, 1,
                       R.L.max_nblk_pts ? (const float*)R.B->d_sums : (const float*)nullptr, R.sums_stride);
  gated_linearize(ctx, R, 0, 1);                               // trial linearisation, energies, decision
  hipLaunchKernelGGL(k_ba_apply, dim3(R.L.max_nblk_res, nwin), b, 0, ctx->stream, R.L.d_arr, 1);                                  // accepted: applyRes
  if (R.L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, gp, b, 0, ctx->stream, R.L.d_arr, 2, 0.f, (float*)nullptr, 0, 2);   // rejected: the points go back,
  gated_linearize(ctx, R, 2, 2);                               //           the restored state is linearised again and its energies kept
  if (R.failed) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipGetLastError());
  R.iteration++;
  return SDSO_OK;
}

static int opt_collect(sdso_ctx* ctx, OptRun& R) {
  const int nwin = (int)R.W.size();
  hipLaunchKernelGGL(k_ba_opt_release, dim3(nwin), dim3(128), 0, ctx->stream, R.L.d_arr, R.B->d_out);
  SDSO_HIP(ctx, hipMemcpyAsync(R.B->h_out, R.B->d_out, sizeof(BaOptOut) * nwin, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

// the closing setEvalPT of the newest frame (FullSystemOptimize.cpp:1018-1024): evaluation point = its current pose, zero state but a / b
static void set_newest_eval_pt(BaWindowDev* W) {
  HostFrame& F = W->frames[W->d.nf - 1];
  double nsz[10] = {0};
  nsz[6] = F.state[6];
  nsz[7] = F.state[7];
  F.setEvalPT(F.PRE_worldToCam, nsz);
}

// the end of FullSystem::optimize (FullSystemOptimize.cpp:993-1041): consume the linearisation at the final state, bring the host
// mirrors up to date, newest frame's setEvalPT, linearizeAll(true)
static int opt_finish(sdso_ctx* ctx, OptRun& R, sdso_ba_opt_result_t* out) {
  const int nwin = (int)R.W.size(), nf = R.L.nf;
  int rc = SDSO_OK;
  if (!R.gated) {   // (the gated loop leaves every window linearised at its final state)
    launch_fused(ctx, R.L, R.materialize, 1);
    mark_linearized(R.W, R.materialize);
    if ((rc = opt_consume(ctx, R, 1, false, false))) return rc;
  }
  if ((rc = opt_collect(ctx, R))) return rc;
  std::vector<int> its(nwin), resInA(nwin);
  // host mirrors + the tables at the final state: CPU-only per window (numeric nullspaces, adjoints, the gauge projector), spread
  // over host threads for a batch; the H2D enqueues follow on this thread
  auto finalize = [&](int w) {
    BaWindowDev* W = R.W[w];
    const BaOptOut& o = R.B->h_out[w];
    its[w] = o.iterations; resInA[w] = o.resInA;
    W->calib.setValue(o.calib_value);
    for (int f = 0; f < nf; f++) W->frames[f].setState(o.state[f]);
    W->frames[nf - 1].frameEnergyTH = o.frameTH_new;
    set_newest_eval_pt(W);
    build_tables(W, true);
  };
  const int nthreads = std::max(1, std::min({nwin / 4, 16, (int)std::thread::hardware_concurrency()}));
  if (nthreads <= 1) for (int w = 0; w < nwin; w++) finalize(w);
  else {
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; t++) pool.emplace_back([&] { for (int w; (w = next.fetch_add(1)) < nwin;) finalize(w); });
    for (std::thread& t : pool) t.join();
  }
  size_t tb = 0;
  for (BaWindowDev* W : R.W) tb = std::max(tb, (W->tbl_bytes + 255) & ~(size_t)255);
  char* tstage = nullptr;
  if ((rc = stage_reserve(ctx, ba_state(ctx).stage, tb * nwin, &tstage))) return rc;      // released for reuse by the synchronisation of opt_collect below
  for (int w = 0; w < nwin; w++) {
    BaWindowDev* W = R.W[w];
    if ((rc = upload_tables(ctx, W, true, false, true, tstage + tb * w))) return rc;
    if (W->in_batch) H2D(const_cast<BaDev*>(R.L.d_arr) + w, &W->d, sizeof(BaDev));   // the batch's descriptor copy carries the calibration scalars too
    W->accumulated = false;
  }
  hipLaunchKernelGGL(k_ba_linearize, dim3(R.L.max_nblk_res, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr);
  mark_linearized(R.W, false);
  hipLaunchKernelGGL(k_ba_apply, dim3(R.L.max_nblk_res, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr);
  if ((rc = opt_consume(ctx, R, 1, true, false))) return rc;
  // linearizeAll_Reductor(true)'s per-residual bookkeeping (maxRelBaseline, numGoodResiduals; FullSystemOptimize.cpp:62-78) belongs to THIS
  // optimize call: it runs now, once, for every window — not when (and if) somebody asks for the post-state
  hipLaunchKernelGGL(k_ba_post_state, dim3(R.L.max_nblk_res, nwin), dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr, (float*)nullptr, 1);
  SDSO_HIP(ctx, hipGetLastError());
  if ((rc = opt_collect(ctx, R))) return rc;
  for (int w = 0; w < nwin; w++) {
    BaWindowDev* W = R.W[w];
    const BaOptOut& o = R.B->h_out[w];
    W->frames[nf - 1].frameEnergyTH = o.frameTH_new;
    W->resInL = o.resInL;
    sdso_ba_opt_result_t r;
    r.iterations = its[w];
    r.lastEnergy = o.lastEnergy;
    r.resInA = resInA[w];
    r.rmse = sqrtf((float)(o.lastEnergy / (8 * resInA[w])));
    if (out) out[w] = r;
    W->post_valid = true; W->hs_valid = R.keep_hs || R.gated || !tail_enabled() || R.L.alt; W->last_result = r;
  }
  R.active = false;
  return SDSO_OK;
}

static double opt_lambda(int iteration) { double l = 1e-1; for (int i = 0; i < iteration; i++) l *= 0.25; return l; }
static int opt_iterations(int nf, int mnumOptIts) {
  if (nf < 3) mnumOptIts = 20;
  if (nf < 4) mnumOptIts = 15;
  return mnumOptIts;
}

// solveSystem + doStepFromBackup + the loop's host part of iteration R.iteration.  Single rank: ONE launch of the fused tail kernel.
// Sharded windows: tail kernel (stitch, solve, resubstitute, points' step) -> pack -> all-gather -> k_ba_opt_step, as before.
static int opt_solve_step(sdso_ctx* ctx, OptRun& R, double lambda, int orth, bool folded) {
  if (!tail_enabled() || R.L.alt || R.momentum) {   // (momentum: the stepsize / the kept step come between the solve and the step — opt_step)
    launch_solve(ctx, R.L, lambda, orth, folded);
    SDSO_HIP(ctx, hipGetLastError());
    return opt_step(ctx, R);
  }
  const int flags = ((orth & 1) ? TAIL_ORTH : 0) | (R.L.any_lin ? TAIL_TOPL : 0) | (folded ? 0 : TAIL_FOLD) | (R.keep_hs ? TAIL_HS : 0);
  const int nwin = (int)R.W.size();
  const dim3 gp(std::max(R.L.max_nblk_pts, 1), nwin);
  if (!R.exchange) {
    // the points' back-substitution and step inside the tail kernel (TAIL_RESUB) once every CU has a tail workgroup anyway: 143 -> 132 us
    // for the two at 256 windows; below that the separate kernel spreads a window's points over idle CUs (one window: 0.64 against
    // 0.70 ms per optimize).  SDSO_BA_TAIL_RESUB=0 / 1 forces one form (A/B)
    static const int fuse_env = dbg_env("SDSO_BA_TAIL_RESUB") ? atoi(dbg_env("SDSO_BA_TAIL_RESUB")) : -1;
    const bool fuse_resub = fuse_env >= 0 ? fuse_env != 0 : nwin >= (ctx->aux ? ctx->aux_cus : ctx->n_cu);   // (the CUs this launch may use)
    launch_tail(ctx, R.L, lambda, flags | TAIL_STEP | (fuse_resub ? TAIL_RESUB : 0), R.iteration, 0, R.stop);
    if (R.L.max_nblk_pts && !fuse_resub) { ProfScope ps(ctx, "k_ba_resub", 2); LAUNCH_RESUB_STEP(R.L, gp, dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr, R.iteration + 1, (float*)nullptr, 0); }
    SDSO_HIP(ctx, hipGetLastError());
    R.iteration++;
    return SDSO_OK;
  }
  BaBatch* Bt = R.W[0]->in_batch ? get_batch(ctx) : nullptr;
  if (Bt && Bt->scattered) {
    // reduce-scatter exchange: this rank holds the summed accumulators of its own windows only — it solves those, and the solutions
    // (x, xAd, nres: one record per window) go round by all-gather; every rank then steps its own points of every window, as below
    Bt->scattered = false;
    const int per = nwin / R.nranks, first = comm_rank(ctx) * per;
    BaLaunch own = R.L;
    own.d_arr = R.L.d_arr + first; own.nwin = per;
    launch_tail(ctx, own, lambda, flags);
    const size_t rf = (size_t)sol_rec_floats(R.L.n, R.L.nf);
    SDSO_HIP(ctx, R.B->d_solrec.reserve(ctx->stream, rf * nwin, rf * nwin));
    int rc;
    hipLaunchKernelGGL(k_ba_sol_record, dim3(nwin), dim3(256), 0, ctx->stream, R.L.d_arr, first, per, R.B->d_solrec, 0);
    if ((rc = comm_allgather_floats(ctx, R.B->d_solrec + rf * first, R.B->d_solrec, rf * per))) return rc;
    hipLaunchKernelGGL(k_ba_sol_record, dim3(nwin), dim3(256), 0, ctx->stream, R.L.d_arr, first, per, R.B->d_solrec, 1);
  } else
    launch_tail(ctx, R.L, lambda, flags);
  if (R.L.max_nblk_pts) LAUNCH_RESUB_STEP(R.L, gp, dim3(BA_BLOCK), 0, ctx->stream, R.L.d_arr, -1, R.B->d_sums, R.sums_stride);
  const int rc = opt_consume(ctx, R, 0, false, R.L.max_nblk_pts > 0);
  R.iteration++;
  return rc;
}
// one whole GN iteration: accumulate (fused linearisation + Schur part) -> [all-reduce] -> solve + step
static int opt_iteration(sdso_ctx* ctx, OptRun& R, int it) {
  BaBatch* Bt = R.W[0]->in_batch ? get_batch(ctx) : nullptr;
  const bool defer = tail_enabled() && !R.L.alt && !R.exchange && !(Bt && Bt->eager_fold);
  bool folded = launch_fused(ctx, R.L, R.materialize, 3, defer);
  mark_linearized(R.W, R.materialize);
  if (Bt) Bt->folded = folded;
  if (R.exchange) {
    int rc = Bt ? sdso_ba_allreduce(ctx) : SDSO_ERR_STATE;
    if (rc) return rc;
    folded = true;
  }
  const int sm = R.W[0]->solverMode;
  return opt_solve_step(ctx, R, solver_lambda(sm, opt_lambda(it)), solver_orth_x(sm, it >= 2) ? 1 : 0, folded);
}

// the iterations of a begun loop, single window or batch: the gated start and gated iterations, or the plain iterations (the caller finishes)
static int opt_run_iterations(sdso_ctx* ctx, OptRun& R, int mnumOptIts) {
  const int N = opt_iterations(R.L.nf, mnumOptIts);
  int rc;
  if (R.gated && (rc = opt_gated_start(ctx, R))) return rc;
  for (int it = 0; it < N; it++)
    if ((rc = R.gated ? opt_gated_iteration(ctx, R, it) : opt_iteration(ctx, R, it))) return rc;
  return SDSO_OK;
}

static int optimize_resident_single(sdso_ctx* ctx, BaWindowDev* W, int mnumOptIts, sdso_ba_opt_result_t* res) {
  OptRun R;
  R.L = single(W); R.W = {W};
  // RawResidualJacobian records on demand: nothing inside the loop reads the records of a residual that is being re-linearised (the
  // accumulators take them from registers; linearised residuals keep the records fixLinearizationF saw), and the closing
  // linearizeAll(true) — k_ba_linearize + k_ba_apply in opt_finish — writes the records of the final state, which is what
  // PointFrameResidual::J / EFResidual::J hold when FullSystem::optimize returns.  296 B less store traffic per residual and iteration.
  R.materialize = false; R.keep_hs = true;
  // refused before anything is touched: opt_begin would already issue a collective and reset the window's residuals
  if (comm_nranks(ctx) > 1) return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_ba_optimize is a single-rank call; sharded windows use sdso_ba_batch_optimize");
  R.local_only = true;
  int rc = opt_begin(ctx, R, 1);
  if (rc) return rc;
  if ((rc = opt_run_iterations(ctx, R, mnumOptIts))) return rc;
  return opt_finish(ctx, R, res);
}
// sdso_ba_allreduce asks: is this exchange the reduce-scatter by window?  Only inside the accepted-step resident loop of a sharded batch
// whose windows divide over the ranks, with the fused tail kernel, and without lastHS / lastbS being kept (they exist on the solving
// rank only); anything else takes the all-reduce, whatever mode the batch carries.
// The decision itself is taken ONCE, in sdso_ba_batch_optimize_begin, from this rank's state AND agreed on by all ranks (opt_begin:
// ranks that disagree — another exchange mode, SDSO_BA_TAIL, keep_system — would issue ncclReduceScatter against ncclAllReduce and hang).
static OptRun* get_run(sdso_ctx* ctx) { return ctx && ctx->ba ? ctx->ba->run : nullptr; }
bool ba_batch_scatter_wanted(sdso_ctx* ctx) {
  BaBatch* Bt = get_batch(ctx);
  OptRun* R = get_run(ctx);
  return Bt && R && R->active && R->scatter && R->W == Bt->W;
}
void ba_batch_scatter_done(sdso_ctx* ctx) {
  if (BaBatch* Bt = get_batch(ctx)) Bt->scattered = true;
}
void free_optrun(sdso_ctx* ctx) {
  if (ctx->ba) { delete ctx->ba->run; ctx->ba->run = nullptr; }
}
}  // namespace sdso

// FullSystem::optimize, DSO-native GN loop (FullSystemOptimize.cpp:871-1041)
extern "C" int sdso_ba_optimize(sdso_ctx* ctx, int win, int mnumOptIts, double* state_out, float* idepth_out, uint8_t* res_state_out, sdso_ba_opt_result_t* out) {
  GET_WIN();
  const int nf = W->d.nf, np = W->d.np, nr = W->d.nr;
  sdso_ba_opt_result_t res{0, 0, 0, 0};
  BaLaunch L = single(W);
  // The whole loop runs on the device (ba_opt.hip) without a host round trip: the accepted-step flow (setting_forceAceptStep, the
  // reference's default) through the fused kernel, the energy-gated flow through the un-fused ones with the decision taken by
  // k_ba_opt_gate.  The SVD / orthogonalised-system solver modes and SDSO_BA_HOST_LOOP=1 (A/B) take the host loop below.
  const bool host_loop = dbg_env("SDSO_BA_HOST_LOOP") != nullptr;   // read per call: tests flip it
  if (nf >= 2 && !host_loop && (!solver_alt(W->solverMode) || !solve_on_host())) {
    int rc = optimize_resident_single(ctx, W, mnumOptIts, &res);
    if (rc) return rc;
  } else if (nf >= 2) {
    mnumOptIts = opt_iterations(nf, mnumOptIts);
    hipLaunchKernelGGL(k_ba_reset_all, dim3(L.max_nblk_res, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
    double lastEnergy = 0;
    int rc = linearize_all(ctx, W, false, &lastEnergy);
    if (rc) return rc;
    double lastEnergyL = 0, lastEnergyM = 0;
    rc = calc_energies(ctx, W, &lastEnergyL, &lastEnergyM);
    if (rc) return rc;
    launch_apply(ctx, L);
    double lambda = 1e-1;
    float stepsize = 1;
    const bool momentum = (W->solverMode & SOLVER_MOMENTUM) != 0;
    std::vector<double> x, previousX(W->d.n, std::numeric_limits<double>::quiet_NaN());
    std::vector<float> sums(2 * (W->nblk_pts + 1));
    for (int iteration = 0; iteration < mnumOptIts; iteration++) {
      res.iterations++;
      // backupState(iteration != 0) (:309-351); SOLVER_MOMENTUM also keeps the previous steps (the points': k_ba_resub, which looks at the
      // iteration count of the window's BaOptDev)
      for (int i = 0; i < 4; i++) W->calib.value_backup[i] = W->calib.value[i];
      for (HostFrame& f : W->frames) for (int i = 0; i < 10; i++) { f.step_backup[i] = (momentum && iteration != 0) ? f.step[i] : 0.0; f.state_backup[i] = f.state[i]; }
      W->h_opt.iterations = iteration;
      H2D(&W->d_opt->iterations, &W->h_opt.iterations, sizeof(int));
      if (L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, dim3(L.max_nblk_pts, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 0, 0.f, (float*)nullptr);
      // solveSystem
      launch_accumulate(ctx, L, nullptr, false);
      rc = solve_system(ctx, W, iteration, lambda);
      if (rc) return rc;
      rc = fetch_x(ctx, W, x);
      if (rc) return rc;
      {  // incDirChange and the step size (:933-948)
        double dot = 0, n0 = 0, n1 = 0;
        for (int i = 0; i < W->d.n; i++) { dot += previousX[i] * x[i]; n0 += previousX[i] * previousX[i]; n1 += x[i] * x[i]; }
        const double incDirChange = (1e-20 + dot) / (1e-20 + std::sqrt(n0) * std::sqrt(n1));
        previousX = x;
        if (std::isfinite(incDirChange) && (W->solverMode & SOLVER_STEPMOMENTUM)) {
          const float newStepsize = (float)std::exp(incDirChange * 1.4);
          if (incDirChange < 0 && stepsize > 1) stepsize = 1;
          stepsize = sqrtf(sqrtf(newStepsize * stepsize * stepsize * stepsize));
          if (stepsize > 2) stepsize = 2;
          if (stepsize < 0.25f) stepsize = 0.25f;
        }
      }
      // doStepFromBackup (:207-305)
      double nv[4];
      for (int i = 0; i < 4; i++) nv[i] = W->calib.value_backup[i] + (momentum ? 1.0f : stepsize) * W->calib.step[i];
      W->calib.setValue(nv);
      float sumA = 0, sumB = 0, sumT = 0, sumR = 0;
      for (HostFrame& fh : W->frames) {
        double ns[10], st[10];
        for (int i = 0; i < 10; i++) st[i] = fh.step[i];
        if (momentum) for (int i = 0; i < 6; i++) st[i] += 0.5f * fh.step_backup[i];     // :231
        for (int i = 0; i < 10; i++) ns[i] = fh.state_backup[i] + (momentum ? 1.0 : (double)stepsize) * st[i];
        fh.setState(ns);
        sumA += st[6] * st[6];
        sumB += st[7] * st[7];
        sumT += st[0] * st[0] + st[1] * st[1] + st[2] * st[2];
        sumR += st[3] * st[3] + st[4] * st[4] + st[5] * st[5];
      }
      float sumNID = 0, numID = (float)np;
      if (L.max_nblk_pts) {
        hipLaunchKernelGGL(k_ba_points_op, dim3(L.max_nblk_pts, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 1, stepsize, W->d_sums);
        SDSO_HIP(ctx, hipMemcpyAsync(sums.data(), W->d_sums, sizeof(float) * 2 * W->nblk_pts, hipMemcpyDeviceToHost, ctx->stream));
        SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < W->nblk_pts; b++) sumNID += sums[2 * b + 1];
      }
      sumA /= nf; sumB /= nf; sumR /= nf; sumT /= nf;
      sumNID /= numID;
      rc = upload_tables(ctx, W, false);  // setPrecalcValues
      if (rc) return rc;
      const bool canbreak = sqrtf(sumA) < 0.0005 * 1.2f && sqrtf(sumB) < 0.00005 * 1.2f && sqrtf(sumR) < 0.00005 * 1.2f && sqrtf(sumT) * sumNID < 0.00005 * 1.2f;
      double newEnergy = 0;
      rc = linearize_all(ctx, W, false, &newEnergy);
      if (rc) return rc;
      double newEnergyL = 0, newEnergyM = 0;
      rc = calc_energies(ctx, W, &newEnergyL, &newEnergyM);
      if (rc) return rc;
      if (W->forceAccept || (newEnergy + newEnergyL + newEnergyM < lastEnergy + lastEnergyL + lastEnergyM)) {   // :978
        launch_apply(ctx, L);
        lastEnergy = newEnergy; lastEnergyL = newEnergyL; lastEnergyM = newEnergyM;
        lambda *= 0.25;
      } else {
        // loadSateBackup (:355-370), then re-linearize at the restored state
        W->calib.setValue(W->calib.value_backup);
        for (HostFrame& fh : W->frames) { double bs[10]; for (int i = 0; i < 10; i++) bs[i] = fh.state_backup[i]; fh.setState(bs); }
        if (L.max_nblk_pts) hipLaunchKernelGGL(k_ba_points_op, dim3(L.max_nblk_pts, 1), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 2, 0.f, (float*)nullptr);
        rc = upload_tables(ctx, W, false);
        if (rc) return rc;
        rc = linearize_all(ctx, W, false, &lastEnergy);
        if (rc) return rc;
        rc = calc_energies(ctx, W, &lastEnergyL, &lastEnergyM);
        if (rc) return rc;
        lambda *= 1e2;
      }
      if (canbreak && iteration >= 1) break;
    }
    set_newest_eval_pt(W);
    rc = upload_tables(ctx, W, true);
    if (rc) return rc;
    rc = linearize_all(ctx, W, true, &lastEnergy);
    if (rc) return rc;
    // (one read for resInA and resInL: k_ba_post_state below writes the points' counters and the projections, never the accumulator block)
    if ((rc = read_nres(ctx, W, &res.resInA, &W->resInL))) return rc;
    res.lastEnergy = lastEnergy;
    res.rmse = sqrtf((float)(lastEnergy / (8 * res.resInA)));
    // linearizeAll_Reductor(true)'s per-residual bookkeeping (maxRelBaseline, numGoodResiduals; FullSystemOptimize.cpp:62-78): once per optimize, now
    if (nr) hipLaunchKernelGGL(k_ba_post_state, dim3(std::max(W->nblk_res, 1), 1), dim3(BA_BLOCK), 0, ctx->stream, (const BaDev*)W->d_self, (float*)nullptr, 1);
    SDSO_HIP(ctx, hipGetLastError());
    W->post_valid = true; W->hs_valid = true; W->last_result = res;
  } else {
    // fewer than two keyframes: the reference returns 0 before touching anything (FullSystemOptimize.cpp:873-874)
    W->post_valid = true; W->hs_valid = false; W->last_result = res; W->resInL = 0;
  }
  const int rcs = get_state(ctx, W, state_out, idepth_out, res_state_out);   // (synchronises first)
  if (rcs) return rcs;
  if (out) *out = res;
  return SDSO_OK;
}

// FullSystem::optimize for every window of the batch, device-resident (no host round trip inside the loop):
//   begin : backupState's initial copy of the states on the device, resetOOB of every residual
//   then per iteration  sdso_ba_batch_accumulate -> [sdso_ba_allreduce] -> sdso_ba_batch_solve -> sdso_ba_batch_step
//   end   : the linearisation at the final state, setEvalPT of the newest frame, linearizeAll(true); results per window
// sdso_ba_batch_optimize runs the whole sequence with the reference's lambda / orthogonalisation schedule.
extern "C" int sdso_ba_batch_optimize_begin(sdso_ctx* ctx, int stop_on_convergence) {
  GET_BATCH();
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  free_optrun(ctx);
  OptRun* R = new OptRun();
  R->L = batch_launch(Bt); R->W = Bt->W; R->materialize = Bt->materialize; R->keep_hs = Bt->keep_system;
  R->scatter_local = Bt->exchange_mode == 1;
  int rc = opt_begin(ctx, *R, stop_on_convergence);
  if (rc) { delete R; return rc; }
  ba_state(ctx).run = R;
  return SDSO_OK;
}
extern "C" int sdso_ba_batch_step(sdso_ctx* ctx) {
  OptRun* R = get_run(ctx);
  if (!R) return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_ba_batch_optimize_begin first");
  SDSO_REQUIRE(ctx, get_batch(ctx) && get_batch(ctx)->W == R->W, "the batch changed since sdso_ba_batch_optimize_begin");
  SDSO_REQUIRE(ctx, !R->gated, "sdso_ba_batch_step drives the accepted-step flow; energy-gated windows run through sdso_ba_batch_optimize");
  return opt_step(ctx, *R);
}
// sdso_ba_batch_solve + sdso_ba_batch_step as ONE enqueue: solveSystemF, resubstituteF, doStepFromBackup, setPrecalcValues / setDeltaF /
// setNewFrameEnergyTH and the break test of the batch's resident loop run in one launch of the fused tail kernel (ba_tail.hip)
extern "C" int sdso_ba_batch_solve_step(sdso_ctx* ctx, double lambda, int orthogonalize_x) {
  OptRun* R = get_run(ctx);
  if (!R) return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_ba_batch_optimize_begin first");
  BaBatch* Bt = get_batch(ctx);
  SDSO_REQUIRE(ctx, Bt && Bt->W == R->W, "the batch changed since sdso_ba_batch_optimize_begin");
  SDSO_REQUIRE(ctx, !R->gated, "sdso_ba_batch_solve_step drives the accepted-step flow; energy-gated windows run through sdso_ba_batch_optimize");
  lambda = solver_lambda(Bt->W[0]->solverMode, lambda);
  R->L = batch_launch(Bt);
  AuxScope aux(ctx);
  return opt_solve_step(ctx, *R, lambda, orthogonalize_x ? 1 : 0, Bt->folded);
}
extern "C" int sdso_ba_batch_optimize_end(sdso_ctx* ctx, sdso_ba_opt_result_t* out) {
  OptRun* R = get_run(ctx);
  if (!R) return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_ba_batch_optimize_begin first");
  SDSO_REQUIRE(ctx, get_batch(ctx) && get_batch(ctx)->W == R->W, "the batch changed since sdso_ba_batch_optimize_begin");
  R->L = batch_launch(get_batch(ctx));
  const int rc = opt_finish(ctx, *R, out);
  free_optrun(ctx);
  return rc;
}
extern "C" int sdso_ba_batch_optimize(sdso_ctx* ctx, int mnumOptIts, sdso_ba_opt_result_t* out) {
  if (BaBatch* Bt = get_batch(ctx)) {
    if (solver_alt(Bt->W[0]->solverMode) && solve_on_host()) {
      // SDSO_BA_SOLVE_HOST=1 (A/B): the SVD / orthogonalised-system solver modes host-driven (one round trip per iteration,
      // solve_system_host) — the batch call runs the single-window host loop window by window.  Default: the resident loop below, with
      // k_ba_solve_alt in the place of the tail kernel's stitch and solve
      SDSO_HIP(ctx, hipSetDevice(ctx->device));
      free_optrun(ctx);
      for (size_t i = 0; i < Bt->wins.size(); i++) {
        const int rc = sdso_ba_optimize(ctx, Bt->wins[i], mnumOptIts, nullptr, nullptr, nullptr, out ? &out[i] : nullptr);
        if (rc) return rc;
      }
      Bt->folded = true;
      return SDSO_OK;
    }
  }
  int rc = sdso_ba_batch_optimize_begin(ctx, 1);
  if (rc) return rc;
  if ((rc = opt_run_iterations(ctx, *get_run(ctx), mnumOptIts))) { free_optrun(ctx); return rc; }
  return sdso_ba_batch_optimize_end(ctx, out);
}
