// BA host API, part 2 (included by ba.hip): launches on an array of windows.  BaLaunch (one window: single(); a batch: BaBatch::L), the
// launch_* chains of the linearisation, the accumulation, the stitch and the solve, the deferred folds of a batch, and the rules of
// setting_solverMode that the callers share.  (BaBatch is defined here, next to BaLaunch, and not in ba_batch.hip: ensure_folded, which
// the per-window calls need, looks into it.)
namespace sdso {
struct BaLaunch {
  const BaDev* d_arr; int nwin; int max_nblk_res, max_nblk_pts, max_chunks, max_items, nf, n;
  bool any_lin;   // some window holds linearized residuals -> the mode-1 accumulation has work to do
  bool alt;       // the windows' solverMode takes solveSystemF's SVD / orthogonalised-system branches (ba_solve_alt.hip): never the fused tail kernel
  std::vector<BaWindowDev*> Ws;   // the windows behind d_arr (host bookkeeping of a launch: BaWindowDev::l_dirty)
};
struct BaBatch {
  std::vector<int> wins;
  std::vector<BaWindowDev*> W;   // valid while the batch lives: releasing / re-uploading a member frees the batch first
  DevBuf<BaDev> d_arr;
  DevBuf<float> d_accum;
  BaLaunch L;
  bool materialize = true;
  bool eager_fold = false;       // sdso_ba_batch_accum_dev handed the block's address out: never defer the folds
  bool folded = true;            // the packed accumulator block holds the folded sums of the latest accumulate (false: the top partials and the
                                 // per-host Hcc / bc are still unfolded — the fused tail kernel folds them itself; ensure_folded() for anyone else)
  int exchange_mode = 0;         // sdso_ba_batch_exchange_mode: 0 all-reduce + the solve on every rank, 1 reduce-scatter by window + all-gather of x
  bool scattered = false;        // the latest sdso_ba_allreduce was the reduce-scatter: only this rank's windows hold summed accumulators
  bool keep_system = false;      // sdso_ba_batch_keep_system: the resident loop's solves also write lastHS / lastbS (37 KB per window and iteration)
};
static BaBatch* get_batch(sdso_ctx* ctx) { return ctx && ctx->ba ? ctx->ba->batch : nullptr; }

// ---- the rules of setting_solverMode, each stated once
// solveSystemF's SVD / orthogonalised-system branches (ba_solve_alt.hip, or solve_system_host under SDSO_BA_SOLVE_HOST): the bits, and "some"
static int solver_branch(int mode) { return mode & (SOLVER_SVD | SOLVER_ORTHOGONALIZE_SYSTEM); }
static bool solver_alt(int mode) { return solver_branch(mode) != 0; }
// solveSystem's overrides of lambda (EnergyFunctional.cpp:840-846).  With both bits set SOLVER_FIX_LAMBDA wins.  One caller differs: the
// gated resident loop keeps its lambda on the device (launch_solve's orth bit 1) when solver_own_lambda(), and passes 0 through here.
static double solver_lambda(int mode, double lambda) {
  if (mode & SOLVER_USE_GN) lambda = 0;
  if (mode & SOLVER_FIX_LAMBDA) lambda = 1e-5;
  return lambda;
}
static bool solver_own_lambda(int mode) { return !(mode & (SOLVER_USE_GN | SOLVER_FIX_LAMBDA)); }
// x -= P x (EnergyFunctional.cpp:980): always under SOLVER_ORTHOGONALIZE_X, from iteration 2 on under _X_LATER.  `later`: iteration >= 2
// in the loops and the single-window call; sdso_ba_batch_solve hands its caller's flag in on the alt branch only, and
// sdso_ba_batch_solve_step never asks — its caller's flag goes to the kernel as it is.
static bool solver_orth_x(int mode, bool later) { return (mode & SOLVER_ORTHOGONALIZE_X) || (later && (mode & SOLVER_ORTHOGONALIZE_X_LATER)); }

// BaDev::sol behind the three stitched blocks: x (n), then lastHS (n * n) and lastbS (n)
static double* sol_x(const BaDev& d) { return d.sol + 3 * ((size_t)d.n * d.n + d.n); }
static double* sol_last_hs(const BaDev& d) { return sol_x(d) + d.n; }
static double* sol_last_bs(const BaDev& d) { return sol_last_hs(d) + (size_t)d.n * d.n; }

static void launch_linearize(sdso_ctx* ctx, const BaLaunch& L) {
  ProfScope ps(ctx, "k_ba_linearize");
  hipLaunchKernelGGL(k_ba_linearize, dim3(L.max_nblk_res, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
}
static void launch_apply(sdso_ctx* ctx, const BaLaunch& L) {
  hipLaunchKernelGGL(k_ba_apply, dim3(L.max_nblk_res, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
}
// the back-substitution kernels read the points' L sums (p_out[8..13]) only when linearised residuals exist in the launch
#define LAUNCH_RESUB(L_, ...) do { if ((L_).any_lin) hipLaunchKernelGGL(k_ba_resub<true>, __VA_ARGS__); else hipLaunchKernelGGL(k_ba_resub<false>, __VA_ARGS__); } while (0)
#define LAUNCH_RESUB_STEP(L_, ...) do { if ((L_).any_lin) hipLaunchKernelGGL(k_ba_resub_step<true>, __VA_ARGS__); else hipLaunchKernelGGL(k_ba_resub_step<false>, __VA_ARGS__); } while (0)
// The Schur kernel (one workgroup per host frame and window) and what is left to fold afterwards: Hcc / bc over the hosts, and — with
// fold_top_too — the top partials of the fused kernel.  Returns false when those folds were left to the fused tail kernel (defer_fold).
static bool launch_sc_and_folds(sdso_ctx* ctx, const BaLaunch& L, const uint8_t* pflag, bool marg, bool fold_top_too = false, bool defer_fold = false) {
  const int nf = L.nf;
  const int shift = marg ? 0 : 1, mm = marg ? 1 : 0;
  // the launch's common case — no marginalisation pass, no point filter, no linearized residual — takes the kernel's lean per-point loop
  const bool plain = !marg && !pflag && !L.any_lin;
  int clear_l = 0;
  for (BaWindowDev* W : L.Ws) {
    if (plain && W->l_dirty) clear_l = 1;
    W->l_dirty = !plain;          // (a plain launch with clear_l zeroes the L sums of every point it visits: all of them)
  }
  {
    ProfScope ps(ctx, "k_ba_sc", 2);
    // a wave per host (see the kernel) once the workgroups-per-host form would need more than three rounds of two workgroups per CU;
    // SDSO_BA_SC_WPH=0 / 1 forces one form (A/B)
    static const int wph_env = dbg_env("SDSO_BA_SC_WPH") ? atoi(dbg_env("SDSO_BA_SC_WPH")) : -1;
    const int cus = (ctx->aux && ctx->stream == ctx->aux) ? ctx->aux_cus : ctx->n_cu;     // the CUs this launch may use (CU-partitioned ctx: the aux share)
    const bool wph = wph_env >= 0 ? wph_env != 0 : 2 * nf * L.nwin > 13 * cus;   // (round 6, two workgroups per CU since the f64 accumulators — µs,
                                                                                   //  workgroup / wave form: 128 windows 70 / 76, 192: 101 / 108, 224: 122 / 111, 256: 136 / 120: profiles/r06_sc_batch_ab.txt)
    const dim3 g(wph ? (nf + BA_BLOCK / 64 - 1) / (BA_BLOCK / 64) : nf, L.nwin);
    if (plain) { if (wph) hipLaunchKernelGGL((k_ba_sc_host<true, true>), g, dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, pflag, shift, mm, clear_l);
                 else hipLaunchKernelGGL((k_ba_sc_host<true, false>), g, dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, pflag, shift, mm, clear_l); }
    else { if (wph) hipLaunchKernelGGL((k_ba_sc_host<false, true>), g, dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, pflag, shift, mm, 0);
           else hipLaunchKernelGGL((k_ba_sc_host<false, false>), g, dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, pflag, shift, mm, 0); }
  }
  if (fold_top_too && defer_fold) return false;
  if (fold_top_too) hipLaunchKernelGGL(k_ba_fold_all, dim3(1 + 2 * nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr);
  else hipLaunchKernelGGL(k_ba_fold_hcc, dim3(1, L.nwin), dim3(64), 0, ctx->stream, L.d_arr);
  return true;
}
static void launch_accumulate(sdso_ctx* ctx, const BaLaunch& L, const uint8_t* pflag, bool marg) {
  const int nf = L.nf;
  // the folds run even without a single chunk: they are what clears the top bins of the previous call
  if (!marg) {
    if (L.max_chunks > 0) { ProfScope ps(ctx, "k_ba_accum_top", 2); hipLaunchKernelGGL(k_ba_accum_top, dim3(L.max_chunks, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 0, (const uint8_t*)nullptr); }
    hipLaunchKernelGGL(k_ba_fold_top, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr, 0);
    if (L.any_lin && L.max_chunks > 0) {
      hipLaunchKernelGGL(k_ba_accum_top, dim3(L.max_chunks, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 1, (const uint8_t*)nullptr);
      hipLaunchKernelGGL(k_ba_fold_top, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr, 1);
    } else {
      // accumulateLF_MT over zero linearized residuals: only the priors survive (added in the stitch)
      hipLaunchKernelGGL(k_ba_zero_topL, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr);
    }
  } else {
    if (L.max_chunks > 0) hipLaunchKernelGGL(k_ba_accum_top, dim3(L.max_chunks, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 2, pflag);
    hipLaunchKernelGGL(k_ba_fold_top, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr, 0);
  }
  launch_sc_and_folds(ctx, L, pflag, marg);
}
// linearizeAll + applyRes + accumulateAF in one kernel, then the (normally empty) linearized pass and the Schur part
// returns false when the folds were deferred to the tail kernel (defer_fold)
static bool launch_fused(sdso_ctx* ctx, const BaLaunch& L, bool materialize, int part = 3 /* bit 0: linearize+top, bit 1: Schur+folds */, bool defer_fold = false) {
  const int nf = L.nf;
  if ((part & 1) && L.max_chunks > 0) {
    // a linear grid: the kernel deals (window, chunk) out so that a window's chunks share one XCD (k_ba_lin_fused)
    const dim3 g((unsigned)((L.nwin + 7) / 8 * 8 * L.max_chunks)), b(BA_BLOCK);
    if (materialize) launch_timed(ctx, "k_ba_lin_fused", 1, k_ba_lin_fused<true>, g, b, (const BaDev*)L.d_arr, (int)L.nwin, (int)L.max_chunks);
    else launch_timed(ctx, "k_ba_lin_fused", 1, k_ba_lin_fused<false>, g, b, (const BaDev*)L.d_arr, (int)L.nwin, (int)L.max_chunks);
    if (L.any_lin) {
      hipLaunchKernelGGL(k_ba_fold_top, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr, 0);
      hipLaunchKernelGGL(k_ba_accum_top, dim3(L.max_chunks, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr, 1, (const uint8_t*)nullptr);
      hipLaunchKernelGGL(k_ba_fold_top, dim3(nf * nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr, 1);
    }
  }
  // without linearized residuals the top partials are folded together with the Schur partials, after the Schur kernel
  if (part & 2) return launch_sc_and_folds(ctx, L, nullptr, false, !L.any_lin, defer_fold);
  return true;
}
// stitchDouble of the three accumulator groups: the Schur pre-products, then one wave per output tile
static void launch_stitch(sdso_ctx* ctx, const BaLaunch& L) {
  const int nf = L.nf;
  hipLaunchKernelGGL(k_ba_stitch_pre, dim3((2 * nf * nf + 3) / 4, L.nwin), dim3(256), 0, ctx->stream, L.d_arr);
  const dim3 sg((3 * (nf * nf + nf + 1) + ST_WAVES - 1) / ST_WAVES, L.nwin), sb(64 * ST_WAVES);
  // NF = 0 (runtime nf): the fully unrolled NF = 8 instantiation was measured 2x slower (register pressure: 259 vs 127 us per 64 windows)
  hipLaunchKernelGGL(k_ba_stitch<0>, sg, sb, 0, ctx->stream, L.d_arr);
}
// the fused tail kernel (ba_tail.hip); SDSO_BA_TAIL=0 keeps the chain of separate kernels (A/B)
static bool tail_enabled() { static const bool on = !(dbg_env("SDSO_BA_TAIL") && atoi(dbg_env("SDSO_BA_TAIL")) == 0); return on; }
static void launch_tail(sdso_ctx* ctx, const BaLaunch& L, double lambda, int flags, int iteration = 0, int last = 0, int stop = 0) {
  ProfScope ps(ctx, "k_ba_tail", 2);
  if (L.nf == 8) hipLaunchKernelGGL(k_ba_tail<8>, dim3(L.nwin), dim3(TAIL_NT), 0, ctx->stream, L.d_arr, lambda, flags, iteration, last, stop);
  else hipLaunchKernelGGL(k_ba_tail<0>, dim3(L.nwin), dim3(TAIL_NT), 0, ctx->stream, L.d_arr, lambda, flags, iteration, last, stop);
}
static void launch_fold_deferred(sdso_ctx* ctx, const BaLaunch& L) {   // what launch_fused left out under defer_fold
  hipLaunchKernelGGL(k_ba_fold_all, dim3(1 + 2 * L.nf * L.nf, L.nwin), dim3(128), 0, ctx->stream, L.d_arr);
}
// stitch + solveSystemF (default branch) + resubstitute.  orth bit 0: x -= P x; bit 1: lambda of the window's resident loop.
// folded = false: the accumulate left the folds to the tail kernel (launch_fused with defer_fold)
static bool solve_on_host() { return dbg_env("SDSO_BA_SOLVE_HOST") != nullptr; }   // A/B: the SVD / orthogonalised-system branches through solve_system_host
static void launch_solve(sdso_ctx* ctx, const BaLaunch& L, double lambda, int orth, bool folded = true) {
  const int n = L.n;
  if (L.alt) {   // solveSystemF's SVD / orthogonalised-system branches: stitch, then one workgroup per window (ba_solve_alt.hip)
    if (!folded) launch_fold_deferred(ctx, L);
    launch_stitch(ctx, L);
    hipLaunchKernelGGL(k_ba_solve_alt, dim3(L.nwin), dim3(ALT_NT), 0, ctx->stream, L.d_arr, lambda, orth);
    if (L.max_nblk_pts > 0) LAUNCH_RESUB(L, dim3(L.max_nblk_pts, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
    return;
  }
  if (tail_enabled()) {
    const int flags = TAIL_HS | ((orth & 1) ? TAIL_ORTH : 0) | ((orth & 2) ? TAIL_LAMBDA_DEV : 0) | (L.any_lin ? TAIL_TOPL : 0) | (folded ? 0 : TAIL_FOLD);
    launch_tail(ctx, L, lambda, flags);
    if (L.max_nblk_pts > 0) LAUNCH_RESUB(L, dim3(L.max_nblk_pts, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
    return;
  }
  if (!folded) launch_fold_deferred(ctx, L);
  launch_stitch(ctx, L);
  const size_t lds = sizeof(double) * ((size_t)n * ((n + 2) & ~1) + 6 * n + 16) + sizeof(int) * n;   // matrix, six vectors (+16 pad), perm
  hipLaunchKernelGGL(k_ba_solve, dim3(1, L.nwin), dim3(BA_BLOCK), lds, ctx->stream, L.d_arr, lambda, orth);
  if (L.max_nblk_pts > 0) LAUNCH_RESUB(L, dim3(L.max_nblk_pts, L.nwin), dim3(BA_BLOCK), 0, ctx->stream, L.d_arr);
}
// the packed block of a batch whose latest accumulate deferred its folds: fold now (anyone but the tail kernel reads folded sums)
static void ensure_folded(sdso_ctx* ctx, BaBatch* Bt) {
  if (!Bt || Bt->folded) return;
  launch_fold_deferred(ctx, Bt->L);
  Bt->folded = true;
}
static void ensure_folded_win(sdso_ctx* ctx, BaWindowDev* W) { if (W->in_batch) ensure_folded(ctx, get_batch(ctx)); }
// bookkeeping for sdso_ba_get_linearization: where the latest linearisation's records are (fetch_jacobians)
static void mark_linearized(const std::vector<BaWindowDev*>& Ws, bool fused_materialized) {
  for (BaWindowDev* W : Ws) W->j_inplace_last = fused_materialized && W->d.jfix != 0;
}
static BaLaunch single(BaWindowDev* W) {
  BaLaunch L;
  L.d_arr = W->d_self; L.nwin = 1; L.max_nblk_res = std::max(W->nblk_res, 1); L.max_nblk_pts = W->nblk_pts;
  L.max_chunks = W->d.nchunks; L.max_items = W->d.nitems; L.nf = W->d.nf; L.n = W->d.n;
  L.any_lin = W->has_lin_cached;
  L.alt = solver_alt(W->solverMode);
  L.Ws = {W};
  return L;
}
}  // namespace sdso
