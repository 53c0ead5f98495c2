// BA host API, part 5 (included by ba.hip): batches of windows, one launch per phase.  Lifetime of the ctx's batch, the blocks comm.hip
// reduces, and the sdso_ba_batch_* phase calls (the resident loop over a batch: ba_loop.hip).
namespace sdso {
void free_optrun(sdso_ctx* ctx);    // ba_loop.hip (a resident loop over the batch ends with it)
// Dissolve the ctx's batch: every member window gets its own accumulator block back (host descriptor and its device copy),
// so later per-window calls never touch the freed batch block.
static void free_batch(sdso_ctx* ctx) {
  free_optrun(ctx);   // a resident loop over the batch ends with it
  BaBatch* taken = get_batch(ctx);
  if (!taken) return;
  ctx->ba->batch = nullptr;
  hipStreamSynchronize(ctx->stream);
  for (BaWindowDev* W : taken->W) {
    W->d.accum = W->accum_own;
    W->in_batch = false;
    W->accumulated = false;
    hipMemcpyAsync(W->d_self, &W->d, sizeof(BaDev), hipMemcpyHostToDevice, ctx->stream);
  }
  hipStreamSynchronize(ctx->stream);
  delete taken;   // (its blocks with it)
}
static bool batch_defers_fold(sdso_ctx* ctx, BaBatch* Bt) { (void)ctx; return tail_enabled() && !Bt->eager_fold && !Bt->L.alt; }
}  // namespace sdso

#define GET_BATCH()                 \
  BaBatch* Bt = get_batch(ctx);     \
  if (!Bt) return sdso::fail(ctx, SDSO_ERR_STATE, "no batch")

// ------------------------------------------------------------------ batches of windows (one launch per phase)

extern "C" int sdso_ba_batch_create(sdso_ctx* ctx, int nwin, const int* wins) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, nwin > 0 && wins, "bad batch");
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_batch(ctx);
  // validate every member before anything is registered or rebound
  std::vector<BaWindowDev*> Ws(nwin);
  for (int i = 0; i < nwin; i++) {
    Ws[i] = find_win(ctx, wins[i]);
    SDSO_REQUIRE(ctx, Ws[i], "unknown window in batch");
    SDSO_REQUIRE(ctx, Ws[i]->d.nf == Ws[0]->d.nf, "batch windows must share nf");
    SDSO_REQUIRE(ctx, Ws[i]->solverMode == Ws[0]->solverMode, "batch windows must share solverMode (one lambda per launch)");
    for (int k = 0; k < i; k++) SDSO_REQUIRE(ctx, Ws[k] != Ws[i], "a window may appear only once in a batch");
  }
  const int nf = Ws[0]->d.nf;
  const size_t af = acc_floats(nf);
  DevBuf<BaDev> d_arr;
  DevBuf<float> d_accum;
  SDSO_HIP(ctx, d_arr.reserve(ctx->stream, nwin, nwin));
  SDSO_HIP(ctx, d_accum.reserve(ctx->stream, af * nwin, af * nwin));
  BaBatch* Bt = new BaBatch();
  Bt->d_arr = std::move(d_arr); Bt->d_accum = std::move(d_accum); Bt->W = Ws;
  Bt->wins.assign(wins, wins + nwin);
  ba_state(ctx).batch = Bt;
  hipMemsetAsync(Bt->d_accum, 0, sizeof(float) * af * nwin, ctx->stream);
  std::vector<BaDev> h(nwin);
  BaLaunch L{};
  L.nwin = nwin; L.nf = nf; L.n = Ws[0]->d.n;
  for (int i = 0; i < nwin; i++) {
    BaWindowDev* W = Ws[i];
    W->d.accum = Bt->d_accum + af * i;   // contiguous accumulators: ONE all-reduce covers the batch
    W->in_batch = true;
    h[i] = W->d;
    hipMemcpyAsync(W->d_self, &W->d, sizeof(BaDev), hipMemcpyHostToDevice, ctx->stream);
    L.max_nblk_res = std::max(L.max_nblk_res, std::max(W->nblk_res, 1)); L.max_nblk_pts = std::max(L.max_nblk_pts, W->nblk_pts);
    L.max_chunks = std::max(L.max_chunks, W->d.nchunks); L.max_items = std::max(L.max_items, W->d.nitems);
    W->accumulated = true;
  }
  hipMemcpyAsync(Bt->d_arr, h.data(), sizeof(BaDev) * nwin, hipMemcpyHostToDevice, ctx->stream);
  L.d_arr = Bt->d_arr;
  L.any_lin = false;   // recomputed at every launch (marginalisation may linearize residuals of a member later)
  L.alt = solver_alt(Ws[0]->solverMode);   // (the members of a batch share one solverMode)
  L.Ws = Ws;
  Bt->L = L;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { free_batch(ctx); return sdso::fail(ctx, SDSO_ERR_HIP, "batch descriptor upload failed"); }
  return SDSO_OK;
}
namespace sdso {
// launch descriptor of the batch with the state-dependent flags refreshed
static const BaLaunch& batch_launch(BaBatch* Bt) {
  Bt->L.any_lin = false;
  for (BaWindowDev* W : Bt->W) if (W->has_lin_cached) { Bt->L.any_lin = true; break; }
  return Bt->L;
}
}  // namespace sdso
namespace sdso {
// comm.hip: the blocks the RCCL all-reduce sums in place
void* ba_batch_accum_block(sdso_ctx* ctx, size_t* nfloats) {
  BaBatch* Bt = get_batch(ctx);
  if (!Bt) return nullptr;
  *nfloats = acc_floats(Bt->L.nf) * Bt->wins.size();
  ensure_folded(ctx, Bt);
  return Bt->d_accum;
}
void* ba_window_accum_block(sdso_ctx* ctx, int win, size_t* nfloats) {
  BaWindowDev* W = find_win(ctx, win);
  if (!W) return nullptr;
  *nfloats = acc_floats(W->d.nf);
  W->accumulated = true;
  ensure_folded_win(ctx, W);
  return W->d.accum;
}
}  // namespace sdso
// phase 1 of one GN iteration for every window of the batch: linearize + applyRes + accumulate A/L/SC (enqueue only).
// Inside a single-rank resident loop (sdso_ba_batch_optimize_begin) the folds of the partial sums are left to the fused tail kernel of
// sdso_ba_batch_solve / sdso_ba_batch_solve_step; whoever else looks at the packed block gets it folded first (ensure_folded).
extern "C" int sdso_ba_batch_accumulate(sdso_ctx* ctx) {
  GET_BATCH();
  Bt->scattered = false;
  Bt->folded = launch_fused(ctx, batch_launch(Bt), Bt->materialize, 3, batch_defers_fold(ctx, Bt));
  mark_linearized(Bt->W, Bt->materialize);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
// the two halves of sdso_ba_batch_accumulate as separate enqueues, for callers that overlap batches on several streams: the
// bandwidth-bound linearisation of one batch is best followed immediately by the linearisation of the next one, with the Schur
// accumulation and the folds of the first running underneath it
// CU-partitioned ctx (sdso_ctx_partition_cus): the launches inside the scope go to the ctx's aux stream, ordered behind everything the main
// stream holds so far; at the end of the scope the main stream is ordered behind them again (its next consumer — the next linearisation of
// THIS batch — needs their results anyway; another ctx's linearisation, on its own stream with the same large CU mask, does not wait).
struct AuxScope {
  sdso_ctx* ctx; hipStream_t main = nullptr;
  explicit AuxScope(sdso_ctx* c) : ctx(c) {
    if (!ctx->aux) return;
    hipEventRecord(ctx->ev_main, ctx->stream);
    hipStreamWaitEvent(ctx->aux, ctx->ev_main, 0);
    main = ctx->stream; ctx->stream = ctx->aux;
  }
  ~AuxScope() {
    if (!main) return;
    hipEventRecord(ctx->ev_aux, ctx->aux);
    ctx->stream = main;
    hipStreamWaitEvent(ctx->stream, ctx->ev_aux, 0);
  }
};
extern "C" int sdso_ba_batch_linearize(sdso_ctx* ctx) {
  GET_BATCH();
  launch_fused(ctx, batch_launch(Bt), Bt->materialize, 1);
  mark_linearized(Bt->W, Bt->materialize);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
extern "C" int sdso_ba_batch_schur(sdso_ctx* ctx) {
  GET_BATCH();
  Bt->scattered = false;
  AuxScope aux(ctx);
  Bt->folded = launch_fused(ctx, batch_launch(Bt), Bt->materialize, 2, batch_defers_fold(ctx, Bt));
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
// materialize = 1 (default): every linearization also writes the RawResidualJacobian records to HBM
// (what PointFrameResidual::J holds in the reference); 0: they stay in registers (the solver never
// re-reads them) — 296 B less store traffic per point-residual.
extern "C" int sdso_ba_batch_set_materialize(sdso_ctx* ctx, int materialize) {
  GET_BATCH();
  Bt->materialize = materialize != 0;
  return SDSO_OK;
}
// phase 2: stitch + solve + resubstitute (enqueue only). Between the phases the caller may all-reduce
// the packed accumulators (sdso_ba_batch_accum_dev) across ranks.
extern "C" int sdso_ba_batch_solve(sdso_ctx* ctx, double lambda, int orthogonalize_x) {
  GET_BATCH();
  SDSO_REQUIRE(ctx, !Bt->scattered, "the accumulators were reduce-scattered by window (exchange mode 1): sdso_ba_batch_solve_step consumes them");
  // solveSystem's overrides of lambda (EnergyFunctional.cpp:840-846), as in the single-window call
  const int sm = Bt->W[0]->solverMode;
  lambda = solver_lambda(sm, lambda);
  if (solver_alt(sm) && solve_on_host()) {
    // SDSO_BA_SOLVE_HOST=1 (A/B): solveSystemF's SVD / orthogonalised-system branches (EnergyFunctional.cpp:876-900, 924-965) with the
    // assembly and the eigen-decomposition on the host, window by window (solve_system_host), the back-substitution on the device.  The
    // host mirrors (deltas, projector) are those of the upload.  Default: k_ba_solve_alt for the whole batch (launch_solve).
    ensure_folded(ctx, Bt);
    for (BaWindowDev* W : Bt->W) {
      const int rc = solve_system_host(ctx, W, orthogonalize_x ? 2 : 0, lambda);   // (iteration >= 2 is how the single call spells ORTHOGONALIZE_X_LATER)
      if (rc) return rc;
    }
    return SDSO_OK;
  }
  const bool no_tail = !tail_enabled() || batch_launch(Bt).alt;
  // as the single call spells it for these branches: the argument is "iteration >= 2", the mode decides (EnergyFunctional.cpp:980)
  if (batch_launch(Bt).alt) orthogonalize_x = solver_orth_x(sm, orthogonalize_x != 0) ? 1 : 0;
  launch_solve(ctx, batch_launch(Bt), lambda, orthogonalize_x, Bt->folded);   // (the tail kernel folds for itself: the block stays as it is)
  if (no_tail) Bt->folded = true;
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
extern "C" int sdso_ba_batch_accum_dev(sdso_ctx* ctx, void** dev_ptr, long* nfloats) {
  GET_BATCH();
  ensure_folded(ctx, Bt);
  Bt->eager_fold = true;          // the caller holds the address: every later accumulate leaves folded sums there
  if (dev_ptr) *dev_ptr = Bt->d_accum;
  if (nfloats) *nfloats = (long)(acc_floats(Bt->L.nf) * Bt->wins.size());
  return SDSO_OK;
}
extern "C" int sdso_ba_batch_get_x(sdso_ctx* ctx, double* x /* nwin * (8nf+4) */) {
  GET_BATCH();
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = Bt->L.n;
  for (size_t i = 0; i < Bt->wins.size(); i++) {
    BaWindowDev* W = find_win(ctx, Bt->wins[i]);
    SDSO_HIP(ctx, hipMemcpy(x + i * n, sol_x(W->d), sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return SDSO_OK;
}

extern "C" int sdso_ba_batch_exchange_mode(sdso_ctx* ctx, int mode) {
  GET_BATCH();
  SDSO_REQUIRE(ctx, mode == 0 || mode == 1, "exchange mode: 0 all-reduce, 1 reduce-scatter by window");
  Bt->exchange_mode = mode;
  return SDSO_OK;
}

extern "C" int sdso_ba_batch_keep_system(sdso_ctx* ctx, int on) {
  GET_BATCH();
  Bt->keep_system = on != 0;
  return SDSO_OK;
}

