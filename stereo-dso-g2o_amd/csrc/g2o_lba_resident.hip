// A part of g2o_factors.hip: sdso_g2o_lba_optimize_enqueue / _done / _fetch / _resident — the window optimiser of g2o_lba_opt.hip with
// its Levenberg-Marquardt loop resident on the device.  Same inputs, same rules, same outputs; between enqueue and fetch the host neither
// waits, nor copies, nor decides.
//
// Who does what.  Everything sdso_g2o_lba_optimize keeps on the host between its launches lives in ONE device record, LbaCtl: lambda,
// nu and the chi2 values (g2o_lba::Lm, g2o_lba_core.h), which of the two estimate buffers is current, the current and the tentative
// Twh / affine pairs / camera, the increments, the folded quadratic form, the counters, the stop reason, the recorded trials / lambda /
// chi2, the `done` flag.  The wide kernels are the bodies of k_lba_opt_eval<0/1/2>, k_lba_opt_lin and k_lba_opt_schur (g2o_lba_opt.hip)
// behind a view that takes lambda, the tables, the camera, the idepth buffers and the increments from that record.  Between them runs
// k_lbar_ctl, a single workgroup: it folds the partials in k_lba_opt_fold's order, assembles and solves the block-arrow reduced system
// (g2o_lba::assemble / solve: LbaProblem::trial's assembly and solveLdlt's algorithm), forms exp(x) Twh, a += x6, b += x7, cam += x and
// the float pair tables of the tentative estimate (g2o_lba::pair_table: host_math.h's Se3 product and affFromTo; -ffp-contract=off),
// computeScale's pose part, and takes the LM step.
//
// The schedule is fixed at enqueue and is the loop's upper bound:
//     eval<0>, ctl                                                   the build-time evaluation, the active set
//     max_iterations x { lin,  max_trials x { schur, ctl, eval<2>, ctl },  eval<1>, ctl }
// A launch has one step, named by its place in the schedule; whether that step is needed is decided by the record's phase alone
// (g2o_lba_core.h): a launch whose step is not needed returns at once.  There
// is no flag to wait for, no spin and no grid barrier — ordering comes from the stream — and every loop is bounded by constants or nr.
//
// Determinism: the partial sums, their fold order and the solve's arithmetic are functions of (nf, nr, the host ranges) alone; every
// byte a kernel reads has been written by the upload, a memset or an earlier kernel of the same job.
namespace sdso {

struct LbaCtl {
  g2o_lba::Lm lm;
  int cur, done;                           // which tab[] / idepth[] holds the current estimate; 1 once the phase is PH_DONE
  int nf, nr, nh, n_active;
  int slot[8], n_active_host[8];
  int solved, ev_blocks;
  double scale_pose;                       // computeScale over the pose, photometric and camera increments of the pending trial
  sdso_se3_t Twh[8], Twh_t[8];
  double aff[8][2], aff_t[8][2], cam[4], cam_t[4];
  double x[g2o_lba::kNMax];                // the pending trial's increments by frame index: nf x 8, then the camera's 4
  double A[8][kLbaEnt];                    // the iteration's quadratic form, folded
  // constants of the job
  sdso_se3_t Ttw[8];
  double target_aff[8][2];
  float ab_exposure[8];
  float* tab[2];                           // pair tables {R 9, t 3, ab 2} x nf*nf
  double* idepth[2];
  const double *part_ev, *part_lin, *part_sc;
  const int* hstart;
  const uint8_t* active;
  const float4* img[8];                    // the frames' level-0 images
};
// the launch argument of the wide kernels: LbaOpt with the images named through the record (see LbaDevT)
typedef LbaOptT<LbaDevT<const float4* const*>> LbaOptR;

// the launch's LbaOpt: the job's constants from `base`, what varies from the record.  tentative: the tables and the camera of the trial.
__device__ __forceinline__ LbaOptR lbar_view(const LbaOptR& base, const LbaCtl* __restrict__ c, bool tentative) {
  LbaOptR O = base;
  const int cur = c->cur, which = tentative ? cur ^ 1 : cur;
  const size_t nn = (size_t)base.L.nf * base.L.nf;
  float* tab = c->tab[which];
  O.L.pair_R = tab; O.L.pair_t = tab + nn * 9; O.L.pair_ab = tab + nn * 12;
#pragma unroll
  for (int k = 0; k < 4; k++) O.L.cam[k] = tentative ? c->cam_t[k] : c->cam[k];
  O.idepth_cur = c->idepth[cur]; O.idepth_trial = c->idepth[cur ^ 1];
  O.lambda = c->lm.lambda;
  O.x = c->x;
  return O;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_lbar_eval(LbaOptR base, const LbaCtl* __restrict__ ctl) {
  const int phase = ctl->lm.phase;
  if (phase != (MODE == 0 ? g2o_lba::PH_INIT : MODE == 1 ? g2o_lba::PH_TERM_EVAL : g2o_lba::PH_TRIAL_EVAL)) return;
  base.part = const_cast<double*>(ctl->part_ev);
  lba_opt_eval_body<MODE>(lbar_view(base, ctl, MODE == 2));
}
__global__ __launch_bounds__(256) void k_lbar_lin(LbaOptR base, const LbaCtl* __restrict__ ctl) {
  if (ctl->lm.phase != g2o_lba::PH_HEAD) return;
  base.part = const_cast<double*>(ctl->part_lin);
  lba_opt_lin_body(lbar_view(base, ctl, false));
}
__global__ __launch_bounds__(128) void k_lbar_schur(LbaOptR base, const LbaCtl* __restrict__ ctl) {
  const int phase = ctl->lm.phase;
  if (phase != g2o_lba::PH_HEAD && phase != g2o_lba::PH_TRIAL) return;
  base.part = const_cast<double*>(ctl->part_sc);
  lba_opt_schur_body(lbar_view(base, ctl, false));
}

constexpr int LBAR_CTL_THREADS = 256;
struct LbarWg {
  __device__ int tid() const { return threadIdx.x; }
  __device__ int nt() const { return LBAR_CTL_THREADS; }
  __device__ void sync() const { __syncthreads(); }
};

// the sum of the evaluation's partials, k_lba_opt_fold's order
__device__ __forceinline__ double lbar_fold_ev(const LbaCtl* c, int v) {
  double s = 0;
  for (int p = 0; p < c->ev_blocks; p++) s += c->part_ev[p * 2 + v];
  return s;
}

// the controller's place in the schedule: after the build-time evaluation, after a Schur complement, after a trial's evaluation, after
// the terminate action's evaluation
enum LbarStep { LBAR_START = 0, LBAR_SOLVE = 1, LBAR_TRIAL = 2, LBAR_TERM = 3 };

__global__ __launch_bounds__(LBAR_CTL_THREADS) void k_lbar_ctl(LbaCtl* __restrict__ ctl, int step) {
  const int phase = ctl->lm.phase;           // (uniform; thread 0 moves it at the very end of a step)
  const bool mine = step == LBAR_START ? phase == g2o_lba::PH_INIT
                  : step == LBAR_SOLVE ? (phase == g2o_lba::PH_HEAD || phase == g2o_lba::PH_TRIAL)
                  : step == LBAR_TRIAL ? phase == g2o_lba::PH_TRIAL_EVAL : phase == g2o_lba::PH_TERM_EVAL;
  if (!mine) return;
  const int tid = threadIdx.x, nf = ctl->nf;
  if (phase == g2o_lba::PH_INIT) {           // the build-time evaluation has run: the active set per host, the controller's start
    __shared__ int s_cnt[8];
    if (tid < 8) s_cnt[tid] = 0;
    __syncthreads();
    for (int h = 0; h < nf; h++) {
      int c = 0;
      for (int i = ctl->hstart[h] + tid; i < ctl->hstart[h + 1]; i += LBAR_CTL_THREADS) c += ctl->active[i] != 0;
      if (c) atomicAdd(&s_cnt[h], c);
    }
    __syncthreads();
    if (tid == 0) {
      int n_active = 0;
      for (int h = 0; h < 8; h++) { ctl->n_active_host[h] = h < nf ? s_cnt[h] : 0; n_active += ctl->n_active_host[h]; }
      ctl->n_active = n_active;
      ctl->nh = g2o_lba::make_slots(ctl->n_active_host, nf, ctl->slot);
      const g2o_lba::Lm& p = ctl->lm;
      ctl->lm.start(p.max_iterations, p.lambda_init, p.gain_threshold, p.max_trials, lbar_fold_ev(ctl, 0), n_active > 0);
      if (ctl->lm.phase == g2o_lba::PH_DONE) ctl->done = 1;
    }
    return;
  }
  if (phase == g2o_lba::PH_TRIAL_EVAL) {     // the tentative estimate has been evaluated: the LM step
    if (tid == 0) {
      const double chi = lbar_fold_ev(ctl, 0), scale_l = lbar_fold_ev(ctl, 1);
      ctl->lm.trial_result(ctl->solved != 0, chi, ctl->scale_pose + scale_l);
      if (ctl->lm.accepted) {
        for (int h = 0; h < nf; h++) { ctl->Twh[h] = ctl->Twh_t[h]; ctl->aff[h][0] = ctl->aff_t[h][0]; ctl->aff[h][1] = ctl->aff_t[h][1]; }
        for (int k = 0; k < 4; k++) ctl->cam[k] = ctl->cam_t[k];
        ctl->cur ^= 1;
      }
    }
    return;
  }
  if (phase == g2o_lba::PH_TERM_EVAL) {      // the terminate action's evaluation has run
    if (tid == 0) {
      ctl->lm.eval_result(lbar_fold_ev(ctl, 0));
      if (ctl->lm.phase == g2o_lba::PH_DONE) ctl->done = 1;
    }
    return;
  }
  // PH_HEAD / PH_TRIAL: the Schur complement at lambda has run (and, at the head of an iteration, the linearisation before it)
  __shared__ double sH[g2o_lba::kNMax * g2o_lba::kNMax];
  __shared__ double sA[8 * kLbaEnt], sS[8 * kLbaEnt];
  __shared__ double s_bf[g2o_lba::kNMax], s_br[g2o_lba::kNMax], s_x[g2o_lba::kNMax], s_D[g2o_lba::kNMax], s_y[g2o_lba::kNMax], s_d0[g2o_lba::kNMax];
  __shared__ int s_p[g2o_lba::kNMax], s_piv[g2o_lba::kNMax], s_flag;
  const int nh = ctl->nh, n = 8 * nh + 4;
  const double lambda = ctl->lm.lambda;
  for (int k = tid; k < nf * kLbaEnt; k += LBAR_CTL_THREADS) {
    const int h = k / kLbaEnt, ent = k % kLbaEnt;
    double a;
    if (phase == g2o_lba::PH_HEAD) {
      a = 0;
      for (int p = 0; p < 2 * kLbaLinChunks; p++) a += ctl->part_lin[((size_t)h * (2 * kLbaLinChunks) + p) * kLbaEnt + ent];
      ctl->A[h][ent] = a;
    } else a = ctl->A[h][ent];
    sA[k] = a;
    double s = 0;
    for (int p = 0; p < kLbaScChunks; p++) s += ctl->part_sc[((size_t)h * kLbaScChunks + p) * kLbaEnt + ent];
    sS[k] = s;
  }
  __syncthreads();
  const LbarWg wg;
  g2o_lba::assemble(wg, sA, sS, ctl->slot, nf, nh, lambda, sH, s_bf, s_br);
  const bool solved = g2o_lba::solve(wg, n, sH, s_br, s_x, s_D, s_y, s_d0, s_p, s_piv, &s_flag);
  // the tentative estimate: exp(x) Twh, a += x6, b += x7 per host with a slot, cam += x (dso_g2o_vertex.cpp:15-18, :30-40, :100-106)
  if (tid < nf) {
    const int h = tid, sl = ctl->slot[h];
    double xh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { xh[k] = sl >= 0 ? s_x[8 * sl + k] : 0.0; ctl->x[h * 8 + k] = xh[k]; }
    ctl->Twh_t[h] = ctl->Twh[h]; ctl->aff_t[h][0] = ctl->aff[h][0]; ctl->aff_t[h][1] = ctl->aff[h][1];
    if (sl >= 0) {
      const Se3 T = expSe3(xh) * se3_from_abi(ctl->Twh[h]);
      se3_to_abi(T, ctl->Twh_t[h]);
      ctl->aff_t[h][0] += xh[6]; ctl->aff_t[h][1] += xh[7];
    }
  }
  if (tid == 64) {
    for (int k = 0; k < 4; k++) { ctl->x[nf * 8 + k] = s_x[8 * nh + k]; ctl->cam_t[k] = ctl->cam[k] + s_x[8 * nh + k]; }
    ctl->scale_pose = g2o_lba::scale_of(s_x, s_bf, n, lambda);
    ctl->solved = solved ? 1 : 0;
  }
  __syncthreads();                           // (the tentative estimate is visible to the workgroup)
  if (tid < nf * nf) {
    const int h = tid / nf, tg = tid % nf;
    const size_t nn = (size_t)nf * nf;
    float* tab = ctl->tab[ctl->cur ^ 1];
    g2o_lba::pair_table(se3_from_abi(ctl->Ttw[tg]), se3_from_abi(ctl->Twh_t[h]), ctl->ab_exposure[h], ctl->ab_exposure[tg], ctl->aff_t[h][0], ctl->aff_t[h][1],
                        ctl->target_aff[tg][0], ctl->target_aff[tg][1], tab + (size_t)tid * 9, tab + nn * 9 + (size_t)tid * 3, tab + nn * 12 + (size_t)tid * 2);
  }
  __syncthreads();                           // (every thread has read the phase and the record before thread 0 moves it)
  if (tid == 0) ctl->lm.trial_proposed();
}

// W, P, S0 validated, sorted, copied into the job's buffers and the whole run enqueued; `out` is checked where the caller has one
static int lbar_enqueue(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, const sdso_g2o_lba_state_t* S,
                        const sdso_g2o_lba_result_t* out, bool want_out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->g2o && ctx->g2o->lbar.pending) return fail(ctx, SDSO_ERR_STATE, "a window optimisation is pending: fetch it first");
  LbaCall call;
  SDSO_TRY(lba_validate(ctx, W, P, S, out, want_out, &call));
  const int nf = W->nf, nr = W->nr;
  if (!ctx->g2o) ctx->g2o = new G2oState();
  LbaResJob& J = ctx->g2o->lbar;
  J.nf = nf; J.nr = nr; J.empty = nr == 0;
  if (nr == 0) { J.pending = true; return SDSO_OK; }
  // one device block: [ctl, tables 0, constants, sorted inputs, idepth 0 | idepth 1, results | tables 1, records, partials]
  const size_t nn = (size_t)nf * nf;
  const int ev_blocks = std::min(kLbaEvalBlocks, (nr + 31) / 32);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_ctl = take(sizeof(LbaCtl)), o_tab0 = take(sizeof(float) * nn * 14), o_b0 = take(sizeof(double) * nf), o_eth = take(sizeof(float) * nf),
               o_hs = take(sizeof(int) * 9), o_host = take(sizeof(int) * nr), o_tg = take(sizeof(int) * nr), o_u = take(sizeof(float) * nr),
               o_v = take(sizeof(float) * nr), o_col = take(sizeof(float) * 8 * nr), o_w = take(sizeof(float) * 8 * nr), o_id0 = take(sizeof(double) * nr);
  const size_t up_bytes = off;
  const size_t o_id1 = take(sizeof(double) * nr), o_act = take(nr), o_lv = take(nr), o_st = take(nr), o_en = take(sizeof(float) * 2 * nr),
               o_cpt = take(sizeof(float) * 3 * nr), o_ih = take(sizeof(float) * nr);
  const size_t res_bytes = off - o_id0;
  const size_t o_tab1 = take(sizeof(float) * nn * 14), o_rec = take(sizeof(double) * kLbaRec * (size_t)nr), o_pev = take(sizeof(double) * 2 * kLbaEvalBlocks),
               o_plin = take(sizeof(double) * nf * 2 * kLbaLinChunks * kLbaEnt), o_psc = take(sizeof(double) * nf * kLbaScChunks * kLbaEnt);
  const size_t dev_bytes = off, down_ctl = (sizeof(LbaCtl) + 255) & ~(size_t)255;
  J.perm.resize(nr);
  SDSO_HIP(ctx, J.dev.reserve(ctx->stream, dev_bytes, dev_bytes + dev_bytes / 4 + 4096));
  SDSO_HIP(ctx, J.up.reserve(ctx->stream, up_bytes, up_bytes + up_bytes / 4 + 4096));
  SDSO_HIP(ctx, J.down.reserve(ctx->stream, down_ctl + res_bytes, down_ctl + res_bytes + res_bytes / 4 + 4096));
  if (!J.ev) SDSO_HIP(ctx, hipEventCreateWithFlags(&J.ev, hipEventDisableTiming));
  J.d_ctl = 0; J.d_res = down_ctl;
  char* base = (char*)J.dev.get();
  char* up = (char*)J.up.get();
  std::memset(up, 0, up_bytes);             // (padding included: the upload's bytes are a function of the inputs alone)
  lba_sort_host_major(W, S->idepth, call.hstart, J.perm.data(),
                      {(int*)(up + o_host), (int*)(up + o_tg), (float*)(up + o_u), (float*)(up + o_v), (float*)(up + o_col), (float*)(up + o_w), (double*)(up + o_id0)});
  std::memcpy(up + o_b0, W->host_b0, sizeof(double) * nf);
  std::memcpy(up + o_eth, W->frameEnergyTH, sizeof(float) * nf);
  std::memcpy(up + o_hs, call.hstart, sizeof(int) * 9);
  LbaCtl& c = *(LbaCtl*)(up + o_ctl);
  c.lm.phase = g2o_lba::PH_INIT;
  c.lm.max_iterations = P->max_iterations; c.lm.max_trials = P->max_trials; c.lm.lambda_init = P->lambda_init; c.lm.gain_threshold = P->gain_threshold;
  c.nf = nf; c.nr = nr; c.ev_blocks = ev_blocks;
  for (int f = 0; f < nf; f++) {
    c.Twh[f] = S->Twh[f]; c.Twh_t[f] = S->Twh[f];
    c.aff[f][0] = c.aff_t[f][0] = S->host_aff[f].a; c.aff[f][1] = c.aff_t[f][1] = S->host_aff[f].b;
    c.Ttw[f] = W->Ttw[f];
    c.target_aff[f][0] = W->target_aff[f].a; c.target_aff[f][1] = W->target_aff[f].b;
    c.ab_exposure[f] = W->ab_exposure[f];
  }
  for (int k = 0; k < 4; k++) c.cam[k] = c.cam_t[k] = S->cam[k];
  c.tab[0] = (float*)(base + o_tab0); c.tab[1] = (float*)(base + o_tab1);
  c.idepth[0] = (double*)(base + o_id0); c.idepth[1] = (double*)(base + o_id1);
  c.part_ev = (const double*)(base + o_pev); c.part_lin = (const double*)(base + o_plin); c.part_sc = (const double*)(base + o_psc);
  c.hstart = (const int*)(base + o_hs); c.active = (const uint8_t*)(base + o_act);
  {   // the pair tables of the estimates as they come in: an input like the others (LbaProblem::tables' text)
    float* tab = (float*)(up + o_tab0);
    for (int h = 0; h < nf; h++)
      for (int tg = 0; tg < nf; tg++) {
        const size_t pr = (size_t)h * nf + tg;
        g2o_lba::pair_table(se3_from_abi(W->Ttw[tg]), se3_from_abi(S->Twh[h]), W->ab_exposure[h], W->ab_exposure[tg], S->host_aff[h].a, S->host_aff[h].b,
                            W->target_aff[tg].a, W->target_aff[tg].b, tab + pr * 9, tab + nn * 9 + pr * 3, tab + nn * 12 + pr * 2);
      }
  }
  for (int f = 0; f < nf; f++) c.img[f] = call.img[f];
  LbaOptR O;
  std::memset(&O, 0, sizeof(O));
  auto& D = O.L;
  D.nf = nf; D.nr = nr; D.w = W->w; D.h = W->h;
  D.img = (const float4* const*)(base + o_ctl + offsetof(LbaCtl, img));
  D.host_b0 = (const double*)(base + o_b0); D.frameEnergyTH = (const float*)(base + o_eth);
  D.host = (const int*)(base + o_host); D.target = (const int*)(base + o_tg); D.u = (const float*)(base + o_u); D.v = (const float*)(base + o_v);
  D.color = (const float*)(base + o_col); D.weights = (const float*)(base + o_w);
  D.state = (uint8_t*)(base + o_st); D.energy = (float*)(base + o_en); D.cpt = (float*)(base + o_cpt); D.idepth_hessian = (float*)(base + o_ih);
  O.hstart = (const int*)(base + o_hs); O.active = (uint8_t*)(base + o_act); O.level = (uint8_t*)(base + o_lv); O.rec = (double*)(base + o_rec);
  LbaCtl* d_ctl = (LbaCtl*)(base + o_ctl);

  SDSO_HIP(ctx, hipMemcpyAsync(base, up, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(base + o_ih, 0, sizeof(float) * nr, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(base + o_id1, 0, sizeof(double) * nr, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(base + o_rec, 0, sizeof(double) * kLbaRec * (size_t)nr, ctx->stream));
  const dim3 g_ev(ev_blocks), g_lin(kLbaLinChunks, nf), g_sc(kLbaScChunks, nf);
  launch_timed(ctx, "k_lbar_eval", 1, k_lbar_eval<0>, g_ev, dim3(256), O, d_ctl);
  launch_timed(ctx, "k_lbar_ctl", 1, k_lbar_ctl, dim3(1), dim3(LBAR_CTL_THREADS), d_ctl, (int)LBAR_START);
  for (int it = 0; it < P->max_iterations; it++) {
    launch_timed(ctx, "k_lbar_lin", 1, k_lbar_lin, g_lin, dim3(256), O, d_ctl);
    for (int q = 0; q < P->max_trials; q++) {
      launch_timed(ctx, "k_lbar_schur", 1, k_lbar_schur, g_sc, dim3(128), O, d_ctl);
      launch_timed(ctx, "k_lbar_ctl", 1, k_lbar_ctl, dim3(1), dim3(LBAR_CTL_THREADS), d_ctl, (int)LBAR_SOLVE);
      launch_timed(ctx, "k_lbar_eval", 1, k_lbar_eval<2>, g_ev, dim3(256), O, d_ctl);
      launch_timed(ctx, "k_lbar_ctl", 1, k_lbar_ctl, dim3(1), dim3(LBAR_CTL_THREADS), d_ctl, (int)LBAR_TRIAL);
    }
    launch_timed(ctx, "k_lbar_eval", 1, k_lbar_eval<1>, g_ev, dim3(256), O, d_ctl);
    launch_timed(ctx, "k_lbar_ctl", 1, k_lbar_ctl, dim3(1), dim3(LBAR_CTL_THREADS), d_ctl, (int)LBAR_TERM);
  }
  SDSO_HIP(ctx, hipGetLastError());
  char* down = (char*)J.down.get();
  SDSO_HIP(ctx, hipMemcpyAsync(down + J.d_ctl, d_ctl, sizeof(LbaCtl), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(down + J.d_res, base + o_id0, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipEventRecord(J.ev, ctx->stream));
  J.pending = true;
  return SDSO_OK;
}

static int lbar_fetch(sdso_ctx* ctx, sdso_g2o_lba_state_t* S, sdso_g2o_lba_result_t* out) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->g2o || !ctx->g2o->lbar.pending) return fail(ctx, SDSO_ERR_STATE, "no window optimisation is pending");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  LbaResJob& J = ctx->g2o->lbar;
  const int nf = J.nf, nr = J.nr;
  SDSO_REQUIRE(ctx, S && out, "null argument");
  SDSO_REQUIRE(ctx, S->Twh && S->host_aff, "null estimate array");
  if (nr > 0) {
    SDSO_REQUIRE(ctx, S->idepth, "null estimate array");
    SDSO_REQUIRE(ctx, out->state && out->energy && out->centerProjectedTo && out->edge_level && out->idepth_hessian && out->active, "null result array");
  }
  if (J.empty) { J.pending = false; lba_result_reset(out); return SDSO_OK; }
  SDSO_HIP(ctx, hipEventSynchronize(J.ev));
  J.pending = false;
  const char* down = (const char*)J.down.get();
  const LbaCtl& c = *(const LbaCtl*)(down + J.d_ctl);
  if (!c.done) return fail(ctx, SDSO_ERR_STATE, "k_lbar_ctl: the run did not end within its schedule");   // (cannot happen)
  // the result block as lbar_enqueue laid it out: idepth 0, idepth 1, active, level, state, energy, centerProjectedTo, idepth_hessian
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_id0 = take(sizeof(double) * nr), o_id1 = take(sizeof(double) * nr), o_act = take(nr), o_lv = take(nr), o_st = take(nr),
               o_en = take(sizeof(float) * 2 * nr), o_cpt = take(sizeof(float) * 3 * nr), o_ih = take(sizeof(float) * nr);
  const char* res = down + J.d_res;
  const double* r_id = (const double*)(res + (c.cur ? o_id1 : o_id0));
  const uint8_t *r_act = (const uint8_t*)(res + o_act), *r_lv = (const uint8_t*)(res + o_lv), *r_st = (const uint8_t*)(res + o_st);
  const float *r_en = (const float*)(res + o_en), *r_cpt = (const float*)(res + o_cpt), *r_ih = (const float*)(res + o_ih);
  const g2o_lba::Lm& R = c.lm;
  for (int i = 0; i < nr; i++) {
    const int r = J.perm[i];
    out->state[r] = r_st[i]; out->edge_level[r] = r_lv[i]; out->active[r] = r_act[i]; out->idepth_hessian[r] = r_ih[i];
    out->energy[r * 2] = r_en[i * 2]; out->energy[r * 2 + 1] = r_en[i * 2 + 1];
    for (int k = 0; k < 3; k++) out->centerProjectedTo[r * 3 + k] = r_cpt[i * 3 + k];
    if (R.iterations > 0) S->idepth[r] = r_id[i];
  }
  if (R.iterations > 0) {
    for (int f = 0; f < nf; f++) {
      if (c.n_active_host[f] == 0) continue;
      S->Twh[f] = c.Twh[f];
      S->host_aff[f].a = c.aff[f][0]; S->host_aff[f].b = c.aff[f][1];
    }
    for (int k = 0; k < 4; k++) S->cam[k] = c.cam[k];
  }
  out->iterations = R.iterations; out->stop = R.stop; out->n_active = c.n_active;
  for (int i = 0; i < SDSO_G2O_LBA_MAX_RECORDED; i++) { out->trials[i] = R.trials[i]; out->lambda[i] = R.lambda_rec[i]; out->chi2[i] = R.chi2_rec[i]; }
  out->chi2_final = R.final_chi2;
  out->rmse = sqrtf((float)(R.final_chi2 / (double)((size_t)8 * (size_t)nr)));   // :867, as sdso_g2o_lba_optimize has it
  return SDSO_OK;
}

}  // namespace sdso

extern "C" int sdso_g2o_lba_optimize_enqueue(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, const sdso_g2o_lba_state_t* S0) {
  return lbar_enqueue(ctx, W, P, S0, nullptr, false);
}
extern "C" int sdso_g2o_lba_optimize_done(sdso_ctx* ctx) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->g2o || !ctx->g2o->lbar.pending) return fail(ctx, SDSO_ERR_STATE, "no window optimisation is pending");
  if (ctx->g2o->lbar.empty) return 1;
  const hipError_t e = hipEventQuery(ctx->g2o->lbar.ev);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }   // an answer, not an error: not what a later hipGetLastError() may report
  return fail(ctx, SDSO_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
}
extern "C" int sdso_g2o_lba_optimize_fetch(sdso_ctx* ctx, sdso_g2o_lba_state_t* S, sdso_g2o_lba_result_t* out) { return lbar_fetch(ctx, S, out); }
extern "C" int sdso_g2o_lba_optimize_resident(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, sdso_g2o_lba_state_t* S,
                                              sdso_g2o_lba_result_t* out) {
  SDSO_TRY(lbar_enqueue(ctx, W, P, S, out, true));
  return lbar_fetch(ctx, S, out);
}
