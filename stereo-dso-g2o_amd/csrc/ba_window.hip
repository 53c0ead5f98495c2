// BA host API, part 1 (included by ba.hip): the device-resident window.  BaWindowDev and the ctx's BA state, the buffer pool, the tables
// derived from the frame states, the upload in its named phases, sdso_ba_keep_projections / sdso_ba_release_window.
namespace sdso {

struct BaBatch;   // ba_launch.hip
struct OptRun;    // ba_loop.hip

struct BaWindowDev {
  BaDev d;                 // host copy of the device descriptor
  BaDev* d_self = nullptr; // device copy (array of 1)
  std::vector<std::pair<void*, size_t>> allocs;
  // host mirror
  HostCalib calib;
  std::vector<HostFrame> frames;
  HostTables tab;
  Dense P;
  std::vector<double> HM, bM;    // host mirror of the marginalisation prior; the MASTER copy is the device's (dt_HM / dt_bM): see hm_host_valid
  bool hm_host_valid = true;     // false: a device kernel changed the prior since the mirror was filled (sync_prior_host brings it up to date)
  double* d_marg = nullptr;      // the prior after sdso_ba_marginalize_frame_dev: marg_dim^2 + marg_dim doubles, adopted by the next window
  double* d_marg2 = nullptr;     // (the other half of the ping-pong when several frames leave at one keyframe)
  int marg_dim = 0;              // its dimension (0: none)
  std::vector<int> marg_frames;  // the window's frames that prior still covers, in order (indices into `frames`)
  bool marg_chain = false;       // the next sdso_ba_marginalize_frame_dev continues from d_marg (no sdso_ba_marginalize_points since the last one)
  bool prior_pristine = false;   // uploaded with HM = bM = NULL and untouched since: what sdso_ba_adopt_prior requires of the adopting window
  int solverMode = 0, forceAccept = 1;
  double affA = 0, affB = 0;
  std::vector<int> perm, inv;     // sorted -> original, original -> sorted
  std::vector<uint8_t> h_target;  // sorted order
  std::vector<int> h_point;       // sorted order
  std::vector<uint8_t> h_lin;     // sorted order mirror of isLinearized
  std::vector<float> h_prior;
  int nblk_res = 0, nblk_pts = 0;
  // device table blocks that are re-uploaded when frame states change
  float* dt_precalc = nullptr; float* dt_adHTdelta = nullptr; float* dt_cdelta = nullptr; float* dt_frameTH = nullptr;
  double* dt_adHost = nullptr; double* dt_adTarget = nullptr; double* dt_prior = nullptr; double* dt_HM = nullptr; double* dt_bM = nullptr; double* dt_P = nullptr;
  float* dt_xAd = nullptr;
  uint8_t* d_pflag = nullptr;
  float* d_sums = nullptr;
  BaOptDev* d_opt = nullptr;    // resident GN loop state (ba_opt.hip)
  BaOptDev h_opt;               // staging of its upload
  std::vector<double> h_prstage;  // staging of the dt_prior upload (upload_tables)
  int newest_first = 0;         // first pair-sorted residual whose target is the newest frame
  char* tbl_first = nullptr;    // the tables upload_tables refreshes are one contiguous block of the window's slab:
  size_t tbl_bytes = 0;         //   [precalc | adHTdelta | cdelta | adHost | adTarget | P | prior | BaDev], 256-byte aligned each
  float* accum_own = nullptr;   // the window's own packed accumulator block (d.accum points into the batch block while batched)
  bool in_batch = false;
  bool accumulated = false;
  bool marg_accumulated = false;  // the packed block holds the sums of the latest sdso_ba_marginalize_points (addPoint<2> + the Schur addPoint of the flagged points)
  bool has_lin_cached = false;  // some residual of the window is linearized (updated wherever h_lin changes)
  bool l_dirty = false;         // p_out's L sums (linearised / marginalised residuals) may be non-zero: the next plain Schur launch clears them
  bool j_inplace_last = false;  // the latest linearisation was the fused kernel's, written IN PLACE into EFResidual::J's slot (BaDev::jfix):
                                // sdso_ba_get_linearization reads the records from there
  // post-state of FullSystem::optimize (sdso_ba_get_post_state)
  bool post_valid = false;      // an optimize call has ended on this window
  bool hs_valid = false;        // the last solveSystemF of that call wrote lastHS / lastbS
  sdso_ba_opt_result_t last_result{0, 0, 0, 0};
  float* d_post = nullptr;      // nr x 19: projectedTo, centerProjectedTo of the closing linearisation
  int resInL = 0, resInM = 0;
  uint8_t* d_flag = nullptr;    // sdso_ba_flag_points: counters, decisions and the staged last_gone (ba_flag.hip), allocated by its first call
  // sdso_ba_window_update: where every frame / point / residual of this window came from (sdso_ba_window_get_order)
  bool has_order = false;
  std::vector<int> ord_frame, ord_point, ord_res;
};

// zeroed device buffer for a window: reuse a pooled buffer of a released window when one of a similar size exists
// (hipMalloc / hipFree of ~40 buffers cost more than the whole upload otherwise)
static int dmalloc(sdso_ctx* ctx, BaWindowDev* W, void** p, size_t bytes, bool zero = true) {
  const size_t want = ((bytes ? bytes : 16) + 255) & ~(size_t)255;
  int best = -1;
  for (int i = 0; i < (int)ctx->ba_pool.size(); i++) {
    const size_t have = ctx->ba_pool[i].second;
    if (have >= want && have <= 2 * want + 4096 && (best < 0 || have < ctx->ba_pool[best].second)) best = i;
  }
  size_t got = want;
  if (best >= 0) { *p = ctx->ba_pool[best].first; got = ctx->ba_pool[best].second; ctx->ba_pool.erase(ctx->ba_pool.begin() + best); }
  else SDSO_HIP(ctx, hipMalloc(p, want));
  if (zero) SDSO_HIP(ctx, hipMemsetAsync(*p, 0, want, ctx->stream));
  W->allocs.emplace_back(*p, got);
  return SDSO_OK;
}
// scratch of the resident loop (ba_loop.hip), one set per ctx, grown on demand
struct OptBufs {
  DevBuf<float> d_sums, d_pack, d_gather, d_lpart, d_solrec;
  DevBuf<BaOptOut> d_out;
  PinBuf<BaOptOut> h_out;
  size_t out_cap = 0;   // windows d_out and h_out both hold: a group (devbuf.h)
};
// the BA state of a ctx besides its windows (sdso_ctx::ba): created by the first call that needs it, freed with the windows
struct BaCtxState {
  StageBuf stage;             // pinned host staging of window uploads and table refreshes (sdso_internal.h), released with the ctx's windows
  BaBatch* batch = nullptr;   // sdso_ba_batch_create
  OptBufs bufs;               // scratch of the resident GN loop
  OptRun* run = nullptr;      // the batch loop in flight between sdso_ba_batch_optimize_begin and _end
};
static BaCtxState& ba_state(sdso_ctx* ctx) { if (!ctx->ba) ctx->ba = new BaCtxState(); return *ctx->ba; }
#define DM(ptr, T, count)                                                   \
  do {                                                                      \
    void* _p = nullptr;                                                     \
    int _rc = dmalloc(ctx, W, &_p, sizeof(T) * (size_t)(count));            \
    if (_rc) return _rc;                                                    \
    ptr = (T*)_p;                                                           \
  } while (0)
#define H2D(dst, src, bytes) SDSO_HIP(ctx, hipMemcpyAsync((void*)(dst), (src), (bytes), hipMemcpyHostToDevice, ctx->stream))

static void free_window(sdso_ctx* ctx, BaWindowDev* W) {
  for (auto& a : W->allocs) {
    if (ctx->ba_pool.size() < 4096) ctx->ba_pool.push_back(a); else hipFree(a.first);
  }
  delete W;
}
static void free_batch(sdso_ctx* ctx);   // ba_batch.hip (a released window may be a member of the ctx's batch)
void release_all_windows(sdso_ctx* ctx) {
  free_batch(ctx);
  if (ctx->ba) { stage_free(ctx->ba->stage); delete ctx->ba; ctx->ba = nullptr; }
  for (auto& kv : ctx->wins) free_window(ctx, kv.second);
  ctx->wins.clear();
}

// the CPU half of upload_tables: everything derived from the frame states / calibration, into the window's own staging members
// (no HIP call: safe to run for several windows on several host threads)
static void build_tables(BaWindowDev* W, bool adjoints) {
  const int nf = W->d.nf, n = W->d.n;
  buildPrecalc(W->calib, W->frames, W->tab);
  if (adjoints) { buildAdjoints(W->frames, W->tab); W->P = buildNullspaceProjector(W->frames); }
  buildDelta(W->calib, W->frames, W->tab);
  std::vector<double>& pr = W->h_prstage;   // member: the copy may still be in flight when upload_tables returns (sync == false)
  pr.assign((size_t)nf * 16 + 4 + n, 0.0);
  for (int f = 0; f < nf; f++)
    for (int i = 0; i < 8; i++) { pr[f * 8 + i] = W->frames[f].prior[i]; pr[nf * 8 + f * 8 + i] = W->frames[f].delta_prior[i]; }
  for (int i = 0; i < 4; i++) pr[nf * 16 + i] = W->tab.cPrior[i];
  for (int i = 0; i < 4; i++) pr[nf * 16 + 4 + i] = (double)W->tab.cDeltaF[i];
  for (int f = 0; f < nf; f++) for (int i = 0; i < 8; i++) pr[nf * 16 + 4 + 4 + f * 8 + i] = W->frames[f].delta[i];
  // calibration scalars live in the descriptor
  W->d.fxl = W->calib.value_scaledf[0]; W->d.fyl = W->calib.value_scaledf[1];
  W->d.cxl = W->calib.value_scaledf[2]; W->d.cyl = W->calib.value_scaledf[3];
  W->d.fxli = W->calib.value_scaledi[0]; W->d.fyli = W->calib.value_scaledi[1];
}
// the eight tables upload_tables refreshes, into a staging area laid out like the device memory from `origin` on (the tables' block for
// upload_tables, the whole slab for the upload)
static void stage_tables(const BaWindowDev* W, char* stage, const char* origin) {
  const int nf = W->d.nf, n = W->d.n;
  auto put = [&](const void* dst, const void* src, size_t bytes) { std::memcpy(stage + ((const char*)dst - origin), src, bytes); };
  put(W->dt_precalc, W->tab.precalc.data(), sizeof(float) * nf * nf * 27);
  put(W->dt_adHTdelta, W->tab.adHTdeltaF.data(), sizeof(float) * nf * nf * 8);
  put(W->dt_cdelta, W->tab.cDeltaF, sizeof(float) * 4);
  put(W->dt_adHost, W->tab.adHost.data(), sizeof(double) * nf * nf * 64);       // unchanged unless `adjoints`: the host copies persist
  put(W->dt_adTarget, W->tab.adTarget.data(), sizeof(double) * nf * nf * 64);
  put(W->dt_P, W->P.a.data(), sizeof(double) * n * n);
  put(W->dt_prior, W->h_prstage.data(), sizeof(double) * W->h_prstage.size());
  put(W->d_self, &W->d, sizeof(BaDev));
}
// tables -> device.  The block is contiguous in the window's slab, so it travels as ONE copy from a pinned staging area: `stage`
// (tbl_bytes of the caller's reservation; it must stay untouched until the stream has passed the copy), or the ctx staging buffer,
// in which case the call synchronises.
static int upload_tables(sdso_ctx* ctx, BaWindowDev* W, bool adjoints, bool sync = true, bool built = false, char* stage = nullptr) {
  if (!built) build_tables(W, adjoints);
  if (!stage) {
    int rc = stage_reserve(ctx, ba_state(ctx).stage, W->tbl_bytes, &stage);
    if (rc) return rc;
    sync = true;
  }
  stage_tables(W, stage, W->tbl_first);
  SDSO_HIP(ctx, hipMemcpyAsync(W->tbl_first, stage, W->tbl_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (sync) SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

// host mirror of the marginalisation prior <- device (the kernels that change it leave the mirror stale)
static int sync_prior_host(sdso_ctx* ctx, BaWindowDev* W) {
  if (W->hm_host_valid) return SDSO_OK;
  const int n = W->d.n;
  SDSO_HIP(ctx, hipMemcpyAsync(W->HM.data(), W->dt_HM, sizeof(double) * n * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(W->bM.data(), W->dt_bM, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  W->hm_host_valid = true;
  return SDSO_OK;
}

static BaWindowDev* find_win(sdso_ctx* ctx, int win) {
  auto it = ctx->wins.find(win);
  return it == ctx->wins.end() ? nullptr : it->second;
}

}  // namespace sdso

using namespace sdso;

#define GET_WIN()                                   \
  if (!ctx) return SDSO_ERR_STATE;                  \
  SDSO_HIP(ctx, hipSetDevice(ctx->device));         \
  BaWindowDev* W = find_win(ctx, win);              \
  SDSO_REQUIRE(ctx, W, "unknown window")

extern "C" int sdso_ba_release_window(sdso_ctx* ctx, int win) {
  if (!ctx) return SDSO_ERR_STATE;
  auto it = ctx->wins.find(win);
  if (it == ctx->wins.end()) return SDSO_OK;
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (it->second->in_batch) free_batch(ctx);   // the batch holds a snapshot of this window's buffers
  free_window(ctx, it->second);
  ctx->wins.erase(it);
  return SDSO_OK;
}

// What sdso_ba_window_update (ba_update.hip) hands to the upload: the window being replaced and, per point / residual of the new window
// (window order), the index in the old one whose device state is carried (< 0: the entry is new and comes from Win like any uploaded one).
// act_rec != nullptr (sdso_ba_window_update_activated): the new entry -1-k of point_src is record act_rec[k] of act_dev, and its float rows are
// filled from that record on the device.
struct WindowCarry {
  BaWindowDev* old; const int* point_src; const int* res_src; const double* prior_H; const double* prior_b; int prior_dim;
  const int* act_rec = nullptr; const ImmActRec* act_dev = nullptr;
};
static void launch_window_gather(sdso_ctx* ctx, const BaWindowDev* W, const WindowCarry& cy, const int* d_psrc, const int* d_rsrc, const int* d_asrc);   // ba_update.hip

// phase times of the upload on stderr under SDSO_BA_UPLOAD_TIMING (diagnostic; tools/dbg_upload_timing.py reads the phase names)
struct UploadTimer {
  const bool on = dbg_env("SDSO_BA_UPLOAD_TIMING") != nullptr;
  std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
  void mark(const char* what) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[sdso_ba_upload_window] %-28s %7.1f us\n", what, std::chrono::duration<double, std::micro>(t - prev).count());
    prev = t;
  }
};

// phase "host mirror of the frames": the descriptor's scalars, calibration, frames and the prior as the host keeps them; the frames'
// tiled level-0 images (imgs)
static int upload_mirror(sdso_ctx* ctx, BaWindowDev* W, const sdso_ba_window_t* Win, std::vector<const char*>& imgs) {
  const int nf = Win->nf, np = Win->np, nr = Win->nr;
  BaDev& d = W->d;
  std::memset(&d, 0, sizeof(d));
  d.nf = nf; d.np = np; d.nr = nr; d.nrp = (nr + 63) & ~63; d.w = Win->w; d.h = Win->h; d.n = 8 * nf + 4;
  d.wM3 = (float)(Win->w - 3); d.hM3 = (float)(Win->h - 3);
  d.affA_fixed = Win->affineOptModeA < 0; d.affB_fixed = Win->affineOptModeB < 0;
  d.jfix = dbg_env("SDSO_BA_JSWAP") && atoi(dbg_env("SDSO_BA_JSWAP")) ? 0 : 1;
  // (every bit of setting_solverMode has its branch: solveSystemF's in launch_solve, STEPMOMENTUM / MOMENTUM in the GN loops, ORTHOGONALIZE_POINTMARG /
  // _FULL in sdso_ba_marginalize_points)
  W->solverMode = Win->solverMode; W->forceAccept = Win->forceAcceptStep; W->affA = Win->affineOptModeA; W->affB = Win->affineOptModeB;
  d.solver_mode = Win->solverMode;
  d.tiledT = tile0_tiles_per_row(Win->w);
  const int n = d.n;
  for (int i = 0; i < 4; i++) W->calib.value_zero[i] = Win->calib_value_zero[i];
  W->calib.setValueScaled(Win->calib_value_scaled);
  W->frames.resize(nf);
  imgs.resize(nf);
  for (int f = 0; f < nf; f++) {
    HostFrame& F = W->frames[f];
    std::memcpy(F.evalPT.R.data(), Win->evalPT + f * 12, 72);
    std::memcpy(F.evalPT.t.data(), Win->evalPT + f * 12 + 9, 24);
    F.ab_exposure = Win->ab_exposure[f]; F.frameEnergyTH = Win->frameEnergyTH[f]; F.frameID = Win->frameID[f]; F.frame_slot = Win->frame_slot[f];
    F.setState(Win->state + f * 10);
    F.setStateZero(Win->state_zero + f * 10);
    for (int i = 0; i < 10; i++) F.step[i] = 0;
    F.fillPrior(W->affA, W->affB, W->solverMode);
    auto ip = ctx->pyr.find(F.frame_slot);
    SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), "window references a frame slot without an uploaded pyramid");
    SDSO_REQUIRE(ctx, ip->second.w[0] == Win->w && ip->second.h[0] == Win->h, "pyramid level-0 size differs from the window's w/h");
    int rc = ensure_tiled0(ctx, ip->second);   // 5x2-tiled 12-byte level-0 images for the linearisation
    if (rc) return rc;
    imgs[f] = ip->second.tiled0;
  }
  W->HM.assign((size_t)n * n, 0.0); W->bM.assign(n, 0.0);
  if (Win->HM) std::memcpy(W->HM.data(), Win->HM, sizeof(double) * n * n);
  if (Win->bM) std::memcpy(W->bM.data(), Win->bM, sizeof(double) * n);
  W->prior_pristine = std::all_of(W->HM.begin(), W->HM.end(), [](double v) { return v == 0.0; }) && std::all_of(W->bM.begin(), W->bM.end(), [](double v) { return v == 0.0; });
  return SDSO_OK;
}

// phase "slab + staging reservation".  Device memory: ONE slab per window.  Segments whose content comes from the host sit at its front and
// are filled by one staged H2D copy (a pinned staging buffer of the ctx, same layout); everything behind them is cleared by one memset.
// (~60 separate buffers with a memset each and ~40 small pageable copies cost 0.7 of the 0.96 ms an upload took.)
struct SlabSeg { void** slot; size_t bytes; bool init; size_t off; };   // where the segment's address goes; init: filled by the staged copy
struct WindowSlab { char* slab = nullptr; char* stage = nullptr; size_t init_bytes = 0, total = 0; int *g_psrc = nullptr, *g_rsrc = nullptr, *g_asrc = nullptr; };
static int upload_lay_out_slab(sdso_ctx* ctx, BaWindowDev* W, bool carry, bool activated, WindowSlab& S) {
  BaDev& d = W->d;
  const int nf = d.nf, np = d.np, nr = d.nr, n = d.n;
  std::vector<SlabSeg> segs;
  segs.reserve(80);
#define PL(ptr, T, count, init) segs.push_back(SlabSeg{(void**)&(ptr), sizeof(T) * (size_t)(count), (init), 0})
  PL(d.p_geo, float4, np, true); PL(d.p_color, float, np * 8, true); PL(d.p_weights, float, np * 8, true); PL(d.p_host, int, np, true);
  PL(d.p_prior, float, np, true); PL(d.p_delta, float, np, true); PL(d.p_rbeg, int, np + 1, true); PL(d.p_rcnt, int, np, true); PL(d.p_rlist, int, nr, true);
  PL(d.p_order, unsigned, np, true); PL(d.p_track, float4, np, true); PL(d.r_isnew, uint8_t, nr, true);
  PL(d.p_out, float, (size_t)np * 16, false); PL(d.p_stepbk, float, np, false);
  PL(d.r_point, int, nr, true); PL(d.r_orig, int, nr, true); PL(d.r_host, uint8_t, nr, true); PL(d.r_target, uint8_t, nr, true);
  PL(d.r_state, uint8_t, nr, true); PL(d.r_newState, uint8_t, nr, false); PL(d.r_lin, uint8_t, nr, false); PL(d.r_act, uint8_t, nr, false); PL(d.r_jsel, uint8_t, nr, false);
  PL(d.r_energy, float, nr, false); PL(d.r_newEnergy, float, nr, false); PL(d.r_newEnergyWO, float, nr, false);
  PL(d.J[0], float, (size_t)76 * d.nrp, false); PL(d.J[1], float, (size_t)76 * d.nrp, false); PL(d.r_toZero, float, (size_t)8 * d.nrp, false);
  PL(d.r_rec, float, (size_t)(nr + 16) * 16, false);  // per-residual records of the Schur part, window order (ba_kernels.h)
  PL(d.r_cj, float, (size_t)(nr + 16) * 8, false);    // their JpJdF halves, compact (written by k_ba_sc_host)
  d.r_proj = nullptr;
  // the tables upload_tables refreshes: contiguous, in this order (one staged copy there too)
  PL(W->dt_precalc, float, nf * nf * 27, true); PL(W->dt_adHTdelta, float, nf * nf * 8, true); PL(W->dt_cdelta, float, 4, true);
  PL(W->dt_adHost, double, nf * nf * 64, true); PL(W->dt_adTarget, double, nf * nf * 64, true); PL(W->dt_P, double, (size_t)n * n, true);
  PL(W->dt_prior, double, nf * 16 + 4 + n, true); PL(W->d_self, BaDev, 1, true);
  PL(W->dt_frameTH, float, nf, true);
  PL(W->dt_HM, double, (size_t)n * n, true); PL(W->dt_bM, double, n, true); PL(W->dt_xAd, float, nf * nf * 8, false);
  PL(d.t_img, const char*, nf, true);
  PL(d.chunks, int4, d.nchunks, true); PL(d.pair_chunk_beg, int, nf * nf + 1, true); PL(d.items, int4, d.nitems, true); PL(d.host_item_beg, int, nf + 1, true);
  PL(d.top_part, double, (size_t)d.nchunks * 92, false); PL(d.sc_part, float, (size_t)nf * 20, false);
  PL(d.e_part, double, std::max(W->nblk_res, d.nchunks) + 1, false);
  PL(d.accum, float, acc_floats(nf), false);
  PL(d.sol, double, sol_doubles(n, nf), false);
  PL(W->d_pflag, uint8_t, np, false); PL(W->d_sums, float, 2 * (W->nblk_pts + 1), false);
  PL(W->d_opt, BaOptDev, 1, false);
  if (carry) { PL(S.g_psrc, int, np, true); PL(S.g_rsrc, int, nr, true); }   // sdso_ba_window_update: the gather maps (pair-sorted for the residuals), staged with the rest
  if (carry && activated) PL(S.g_asrc, int, np, true);                        // sdso_ba_window_update_activated: per point its activation record, or -1
#undef PL
  for (int pass = 0; pass < 2; pass++) {
    for (SlabSeg& sg : segs)
      if (sg.init == (pass == 0)) { sg.off = S.total; S.total += ((sg.bytes ? sg.bytes : 16) + 255) & ~(size_t)255; }
    if (pass == 0) S.init_bytes = S.total;
  }
  void* sp = nullptr;
  int rc = dmalloc(ctx, W, &sp, S.total, false);
  if (rc) return rc;
  S.slab = (char*)sp;
  for (SlabSeg& sg : segs) { char* at = S.slab + sg.off; std::memcpy(sg.slot, &at, sizeof(at)); }   // (the slots are pointers of many types: bytes, not a void* lvalue)
  W->accum_own = d.accum;
  d.opt = W->d_opt; d.finished = 0;
  W->tbl_first = (char*)W->dt_precalc; W->tbl_bytes = (size_t)((char*)W->d_self + sizeof(BaDev) - (char*)W->dt_precalc);
  d.t_precalc = W->dt_precalc; d.t_adHTdelta = W->dt_adHTdelta; d.t_cdelta = W->dt_cdelta; d.t_frameTH = W->dt_frameTH;
  d.t_adHost = W->dt_adHost; d.t_adTarget = W->dt_adTarget; d.t_xAd = W->dt_xAd; d.t_prior = W->dt_prior; d.t_HM = W->dt_HM; d.t_bM = W->dt_bM; d.t_P = W->dt_P;
  if ((rc = stage_reserve(ctx, ba_state(ctx).stage, S.init_bytes, &S.stage))) return rc;
  std::memset(S.stage, 0, S.init_bytes);
  return SDSO_OK;
}

// phase "staging of points / residuals": everything of the staged copy but the tables
static void upload_stage_entries(BaWindowDev* W, const sdso_ba_window_t* Win, const WindowLayout& L, const std::vector<const char*>& imgs, const WindowCarry* carry, const WindowSlab& S) {
  static_assert(sizeof(BaWorkItem) == sizeof(int4), "the work lists are staged as they are built: four ints per entry");
  static_assert(BA_LAYOUT_CHUNK == BA_CHUNK, "ba_layout.h cuts the chunks the accumulate kernels expect");
  const BaDev& d = W->d;
  const int nf = d.nf, np = d.np, nr = d.nr, n = d.n;
  auto put = [&](const void* dst, const void* src, size_t bytes) { std::memcpy(S.stage + ((const char*)dst - S.slab), src, bytes); };
  std::vector<float4> geo(np), track(np);
  W->h_prior.resize(np);
  std::vector<float> delta(np);
  for (int p = 0; p < np; p++) {
    geo[p] = make_float4(Win->u[p], Win->v[p], SCALE_IDEPTH * Win->idepth[p], SCALE_IDEPTH * Win->idepth_zero[p]);
    float pr = Win->hasDepthPrior[p] ? 50.f * 50.f * SCALE_IDEPTH * SCALE_IDEPTH : 0.f;  // EFPoint::takeData, setting_idepthFixPrior
    if (W->solverMode & SOLVER_REMOVE_POSEPRIOR) pr = 0;
    W->h_prior[p] = pr;
    delta[p] = Win->idepth[p] - Win->idepth_zero[p];
    const int ng = Win->numGoodResiduals ? Win->numGoodResiduals[p] : 0;
    float ngf; std::memcpy(&ngf, &ng, 4);
    track[p] = make_float4(Win->maxRelBaseline ? Win->maxRelBaseline[p] : 0.f, ngf, 0.f, 0.f);
  }
  std::vector<uint8_t> isnew(nr, 1);
  if (Win->res_isNew) for (int j = 0; j < nr; j++) isnew[j] = Win->res_isNew[W->perm[j]] ? 1 : 0;
  std::vector<float> frameTH(nf);
  for (int f = 0; f < nf; f++) frameTH[f] = W->frames[f].frameEnergyTH;
  put(d.p_geo, geo.data(), sizeof(float4) * np); put(d.p_color, Win->color, sizeof(float) * np * 8); put(d.p_weights, Win->weights, sizeof(float) * np * 8);
  put(d.p_host, Win->host, sizeof(int) * np); put(d.p_prior, W->h_prior.data(), sizeof(float) * np); put(d.p_delta, delta.data(), sizeof(float) * np);
  put(d.p_rbeg, L.rbeg.data(), sizeof(int) * (np + 1)); put(d.p_rcnt, L.rcnt.data(), sizeof(int) * np);
  put(d.p_rlist, W->inv.data(), sizeof(int) * nr);   // slot order == original order (grouped by point)
  put(d.p_order, L.order.data(), sizeof(unsigned) * np); put(d.p_track, track.data(), sizeof(float4) * np); put(d.r_isnew, isnew.data(), nr);
  put(d.r_point, L.s_point.data(), sizeof(int) * nr); put(d.r_orig, W->perm.data(), sizeof(int) * nr); put(d.r_host, L.s_host.data(), nr); put(d.r_target, L.s_target.data(), nr); put(d.r_state, L.s_state.data(), nr);
  put(W->dt_frameTH, frameTH.data(), sizeof(float) * nf); put(d.t_img, imgs.data(), sizeof(char*) * nf);
  put(d.chunks, L.chunks.data(), sizeof(int4) * L.chunks.size()); put(d.pair_chunk_beg, L.pair_beg.data(), sizeof(int) * (nf * nf + 1));
  put(d.items, L.items.data(), sizeof(int4) * L.items.size()); put(d.host_item_beg, L.host_beg.data(), sizeof(int) * (nf + 1));
  put(W->dt_HM, W->HM.data(), sizeof(double) * n * n); put(W->dt_bM, W->bM.data(), sizeof(double) * n);
  if (carry) {
    std::vector<int> rs(nr);
    for (int j = 0; j < nr; j++) { const int o = carry->res_src[W->perm[j]]; rs[j] = o >= 0 ? carry->old->inv[o] : -1; }
    put(S.g_psrc, carry->point_src, sizeof(int) * np); put(S.g_rsrc, rs.data(), sizeof(int) * nr);
    if (S.g_asrc) {
      std::vector<int> as(np);
      for (int p = 0; p < np; p++) as[p] = carry->point_src[p] < 0 ? carry->act_rec[-1 - carry->point_src[p]] : -1;
      put(S.g_asrc, as.data(), sizeof(int) * np);
    }
  }
}

// carry == nullptr: sdso_ba_upload_window.  Otherwise the old window stays registered and untouched (the caller swaps the two once this
// returned SDSO_OK, or frees *made), and the surviving entries' rows are gathered from its slab after the staged copy.
static int upload_window_impl(sdso_ctx* ctx, int win, const sdso_ba_window_t* Win, const WindowCarry* carry = nullptr, BaWindowDev** made = nullptr) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, Win, "null window");
  const char* why = nullptr;
  if (!window_sizes_ok(*Win, &why)) return sdso::fail(ctx, SDSO_ERR_ARG, why);   // (ahead of the other refusals, as ever; build_window_layout asks again)
  static_assert(TILE0_MAX_BYTES == (size_t)sdso::TAP_RANGE, "the tiled image has to fit the taps' buffer descriptor");
  SDSO_REQUIRE(ctx, Win->w >= 1 && Win->h >= 1 && tile0_bytes(Win->w, Win->h) < TILE0_MAX_BYTES,
               "image size out of range (k_ba_lin_fused reads a tiled level-0 image through a 2 GiB buffer descriptor with 32-bit offsets)");
  SDSO_REQUIRE(ctx, Win->evalPT && Win->state && Win->state_zero && Win->ab_exposure && Win->frameEnergyTH && Win->frameID && Win->frame_slot, "null frame arrays");
  SDSO_REQUIRE(ctx, Win->np == 0 || (Win->u && Win->v && Win->idepth && Win->idepth_zero && Win->color && Win->weights && Win->host && Win->hasDepthPrior), "null point arrays");
  SDSO_REQUIRE(ctx, Win->nr == 0 || (Win->res_point && Win->res_target && Win->res_state), "null residual arrays");
  UploadTimer tm;
  int rc = carry ? SDSO_OK : sdso_ba_release_window(ctx, win);
  if (rc) return rc;
  tm.mark("release of the old window");

  BaWindowDev* W = new BaWindowDev();
  if (made) *made = W;
  if (!carry) ctx->wins[win] = W;
  std::vector<const char*> imgs;
  if ((rc = upload_mirror(ctx, W, Win, imgs))) return rc;
  tm.mark("host mirror of the frames");

  WindowLayout L;   // every validation runs before the first H2D copy
  if (!build_window_layout(*Win, L, &why)) return sdso::fail(ctx, SDSO_ERR_ARG, why);
  BaDev& d = W->d;
  W->perm.swap(L.perm); W->inv.swap(L.inv);
  W->h_target = L.s_target; W->h_point = L.s_point;
  W->h_lin.assign(d.nr, 0);
  W->has_lin_cached = false;
  W->newest_first = L.newest_first;
  d.have_first_frame = L.have_first_frame;
  std::memcpy(d.host_pt_beg, L.host_pt_beg, sizeof(d.host_pt_beg));
  d.nchunks = (int)L.chunks.size();
  d.nitems = (int)L.items.size();
  W->nblk_res = (d.nr + BA_BLOCK - 1) / BA_BLOCK;
  W->nblk_pts = (d.np + BA_BLOCK - 1) / BA_BLOCK;
  tm.mark("validation, sort, work lists");

  WindowSlab S;
  if ((rc = upload_lay_out_slab(ctx, W, carry != nullptr, carry && carry->act_rec, S))) return rc;
  tm.mark("slab + staging reservation");
  upload_stage_entries(W, Win, L, imgs, carry, S);
  tm.mark("staging of points / residuals");
  build_tables(W, true);   // the tables at the uploaded state, staged with everything else
  stage_tables(W, S.stage, S.slab);
  tm.mark("tables (adjoints, projector)");

  SDSO_HIP(ctx, hipMemcpyAsync(S.slab, S.stage, S.init_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (S.total > S.init_bytes) SDSO_HIP(ctx, hipMemsetAsync(S.slab + S.init_bytes, 0, S.total - S.init_bytes, ctx->stream));
  if (carry) launch_window_gather(ctx, W, *carry, S.g_psrc, S.g_rsrc, S.g_asrc);   // the survivors' rows and the prior: old slab -> new slab; activated points: record -> new slab
  // per-residual record: target in slot 15, newState OUTLIER, newEnergyWO -1
  if (d.nr) hipLaunchKernelGGL(k_ba_init_res, dim3(W->nblk_res), dim3(BA_BLOCK), 0, ctx->stream, W->d_self);
  SDSO_HIP(ctx, hipGetLastError());
  // no synchronisation: the upload is ENQUEUED (copy, clear, init kernel) and whatever the caller does next on this ctx queues behind it;
  // the staging buffer is marked in flight (round 5 waited here: 38 of the call's 160 us)
  if ((rc = stage_commit(ctx, ba_state(ctx).stage))) return rc;
  tm.mark("copy + clear + init kernel (enqueue)");
  return SDSO_OK;
}
// a window that failed half-way through its upload must not stay registered (later calls would launch on null arrays)
extern "C" int sdso_ba_upload_window(sdso_ctx* ctx, int win, const sdso_ba_window_t* Win) {
  const int rc = upload_window_impl(ctx, win, Win);
  if (rc && ctx) {
    const std::string why = ctx->err;
    sdso_ba_release_window(ctx, win);
    ctx->err = why;
  }
  return rc;
}

// optional: keep projectedTo / centerProjectedTo (tests); costs 76 B of stores per residual
extern "C" int sdso_ba_keep_projections(sdso_ctx* ctx, int win, int on) {
  if (!ctx) return SDSO_ERR_STATE;
  BaWindowDev* W = find_win(ctx, win);
  SDSO_REQUIRE(ctx, W, "unknown window");
  if (on && !W->d.r_proj) { DM(W->d.r_proj, float, (size_t)W->d.nr * 19); }
  if (!on) W->d.r_proj = nullptr;
  H2D(W->d_self, &W->d, sizeof(BaDev));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

