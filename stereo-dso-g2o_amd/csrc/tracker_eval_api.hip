// The evaluation calls of the coarse tracker: request tables, templates, and calcRes + calcGSSSE for one problem or a batch (part of tracker.hip).
extern "C" void sdso_track_make_eval(const sdso_track_params_t* prm, int lvl, const sdso_se3_t* refToNew, const sdso_aff_t* aff_g2l,
                                     float levelCutoffRepeat, sdso_track_eval_t* ev) {
  fill_eval(*prm, lvl, se3_from_abi(*refToNew), *aff_g2l, prm->coarseCutoffTH * levelCutoffRepeat, *ev);
}

extern "C" int sdso_track_set_ref(sdso_ctx* ctx, int ref_slot, int lvl, int n, const float* pc_u, const float* pc_v,
                                  const float* pc_idepth, const float* pc_color) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, lvl >= 0 && lvl < SDSO_PYR_LEVELS && n >= 0, "bad level / n");
  SDSO_REQUIRE(ctx, n == 0 || (pc_u && pc_v && pc_idepth && pc_color), "null pc arrays");
  RefDev& R = ctx->refs[ref_slot];
  int rc0 = ref_counts(ctx, R);
  if (rc0) return rc0;
  if (R.blk) {
    // the levels are a view of an exported block, which is frozen: the slot detaches.  The call replaces ONE level, so the others come
    // along as copies in buffers of the slot's own (enqueued before share_drop records what this ctx still runs on the block).
    float4* own[SDSO_PYR_LEVELS] = {nullptr};
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) {
      if (l == lvl || R.n[l] <= 0) continue;
      hipError_t e = hipMalloc(&own[l], sizeof(float4) * (size_t)R.n[l]);
      if (e == hipSuccess) e = hipMemcpyAsync(own[l], R.pc[l], sizeof(float4) * (size_t)R.n[l], hipMemcpyDeviceToDevice, ctx->stream);
      if (e != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        for (int k = 0; k < SDSO_PYR_LEVELS; k++) if (own[k]) hipFree(own[k]);
        return sdso::fail(ctx, SDSO_ERR_HIP, std::string("detaching the shared template: ") + hipGetErrorString(e));
      }
    }
    int n_keep[SDSO_PYR_LEVELS];
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) n_keep[l] = R.n[l];
    ref_detach(ctx, R);
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) if (own[l]) { R.pc[l] = own[l]; R.n[l] = R.cap[l] = n_keep[l]; }
  }
  if (R.pc[lvl]) { SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream)); hipFree(R.pc[lvl]); R.pc[lvl] = nullptr; }
  R.n[lvl] = n; R.cap[lvl] = n;
  R.map_ok = R.image_ok = false;   // a template that came from the host has no level-0 map
  if (n == 0) return SDSO_OK;
  std::vector<float4> h(n);
  for (int i = 0; i < n; i++) h[i] = make_float4(pc_u[i], pc_v[i], pc_idepth[i], pc_color[i]);
  SDSO_HIP(ctx, hipMalloc(&R.pc[lvl], sizeof(float4) * (size_t)n));
  SDSO_HIP(ctx, hipMemcpy(R.pc[lvl], h.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
  return SDSO_OK;
}

namespace sdso { void release_g2o_ref(sdso_ctx* ctx, int ref_slot); }   // g2o_factors.hip
extern "C" int sdso_track_release_ref(sdso_ctx* ctx, int ref_slot) {
  if (!ctx) return SDSO_ERR_STATE;
  auto it = ctx->refs.find(ref_slot);
  if (it == ctx->refs.end()) return SDSO_OK;
  // under a pool the levels are parked behind an event on the stream, with no stream synchronisation; what is not pooled (edge sets
  // of the g2o factors, the kept depth map) is freed behind a wait, as ever
  const bool nowait = ctx->pool && !ctx->g2o && !it->second.dmap;
  if (nowait) SDSO_TRY(ref_counts(ctx, it->second));   // (the pinned counts go below: their copy, and nothing else, is waited for)
  else SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  sdso::release_g2o_ref(ctx, ref_slot);
  ref_free(ctx, it->second, !nowait);
  ctx->refs.erase(it);
  return SDSO_OK;
}

static int resolve_prob(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_eval_t& ev, TrackProb& P) {
  TrackLevel L;
  int rc = track_level(ctx, ref_slot, frame_slot, ev.lvl, ev.w, ev.h, &L);
  if (rc) return rc;
  P.ev = ev;
  P.pc = L.pc;
  P.img = L.img;
  P.n = L.n;
  P.pad = 0;
  return SDSO_OK;
}

static int batch_reserve(sdso_ctx* ctx, int nprob, int gx) {
  if (!ctx->tb) ctx->tb = new TrackBatch();
  TrackBatch* tb = ctx->tb;
  if (tb->cap < nprob) {   // two groups (devbuf.h), each with a count of its own
    const size_t cap = (size_t)nprob + nprob / 2 + 8;
    tb->cap = 0;
    SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, tb->d_probs, tb->d_out));
    SDSO_HIP(ctx, tb->d_probs.reserve(ctx->stream, cap, cap));
    SDSO_HIP(ctx, tb->d_out.reserve(ctx->stream, cap, cap));
    tb->cap = (int)cap;
  }
  const size_t need = (size_t)nprob * gx;
  if (tb->part_cap < need) {
    const size_t cap = need + need / 2 + 64;
    tb->part_cap = 0;
    SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, tb->d_partF, tb->d_partI));
    SDSO_HIP(ctx, tb->d_partF.reserve(ctx->stream, TRK_NF * cap, TRK_NF * cap));
    SDSO_HIP(ctx, tb->d_partI.reserve(ctx->stream, TRK_NI * cap, TRK_NI * cap));
    tb->part_cap = cap;
  }
  return SDSO_OK;
}

// workgroups per problem: enough to fill the chip when few problems are in flight.
static int choose_gx(const sdso_ctx* ctx, int nprob, int maxn) {
  if (maxn <= 0) return 1;
  int by_points = (maxn + TRK_BLOCK - 1) / TRK_BLOCK;          // 1 point / thread
  int target = (ctx->n_cu * 8 + nprob - 1) / nprob;            // ~8 workgroups per CU over the batch
  // few, fat workgroups: the per-workgroup epilogue (48-value reduction, partial stores) is amortised over several
  // loop trips (measured on 640 problems: gx 10 -> 65 us, 4 -> 62 us, 1 -> 71 us)
  return std::max(1, std::min(by_points, target));
}

// k_track_eval over `nprob` problems of the ctx's batch buffers at `gx` workgroups each (d_mask: the inlier mask of a single problem, or
// null), then k_track_finalize.  `timed`: the evaluation kernel inside the sdso_prof_* bracket.
static int launch_eval(sdso_ctx* ctx, int nprob, int gx, uint8_t* d_mask, bool timed) {
  TrackBatch* tb = ctx->tb;
  const dim3 grid((nprob + 7) / 8 * 8 * gx), block(TRK_BLOCK);
  auto launch = [&](auto kernel) {
    if (timed) launch_timed(ctx, "k_track_eval", 1, kernel, grid, block, (const TrackProb*)tb->d_probs, nprob, gx, tb->d_partF, tb->d_partI, d_mask);
    else hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, tb->d_probs, nprob, gx, tb->d_partF, tb->d_partI, d_mask);
  };
  if (!d_mask) launch(k_track_eval<false>); else launch(k_track_eval<true>);
  hipLaunchKernelGGL(k_track_finalize, dim3(nprob), dim3(64), 0, ctx->stream, tb->d_probs, tb->d_partF, tb->d_partI, gx, tb->d_out);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}

// One evaluation round trip (the unit of work of the host LM loop): `np` problems in one launch; on return their TrackOuts are at the
// head of ctx->pinned and the stream is idle.  mask_host (np == 1 only): that problem's inlier mask.  Ends any prepared batch.
static int eval_now(sdso_ctx* ctx, const TrackProb* probs, int np, uint8_t* mask_host) {
  int maxn = 0;
  for (int i = 0; i < np; i++) maxn = std::max(maxn, probs[i].n);
  const int gx = choose_gx(ctx, np, maxn);
  int rc = batch_reserve(ctx, np, gx);
  if (rc) return rc;
  TrackBatch* tb = ctx->tb;
  tb->nprob = 0;  // invalidates any prepared batch
  rc = ensure_pinned(ctx, (sizeof(TrackOut) + sizeof(TrackProb)) * (size_t)np);
  if (rc) return rc;
  uint8_t* d_mask = nullptr;
  if (mask_host && probs[0].n > 0) {
    rc = ensure_scratch(ctx, (size_t)probs[0].n);
    if (rc) return rc;
    d_mask = (uint8_t*)ctx->scratch;
  }
  TrackProb* hp = (TrackProb*)((char*)ctx->pinned + sizeof(TrackOut) * (size_t)np);   // staged behind the results
  std::memcpy(hp, probs, sizeof(TrackProb) * np);
  SDSO_HIP(ctx, hipMemcpyAsync(tb->d_probs, hp, sizeof(TrackProb) * np, hipMemcpyHostToDevice, ctx->stream));
  rc = launch_eval(ctx, np, gx, d_mask, false);
  if (rc) return rc;
  SDSO_HIP(ctx, hipMemcpyAsync(ctx->pinned, tb->d_out, sizeof(TrackOut) * np, hipMemcpyDeviceToHost, ctx->stream));
  if (d_mask) SDSO_HIP(ctx, hipMemcpyAsync(mask_host, d_mask, (size_t)probs[0].n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

// result `i` of a call: each array the caller asked for
static void copy_out(const TrackOut& o, size_t i, double* H, double* b, double* res, int* n_warped) {
  if (H) std::memcpy(H + i * 64, o.H, sizeof(double) * 64);
  if (b) std::memcpy(b + i * 8, o.b, sizeof(double) * 8);
  if (res) std::memcpy(res + i * 6, o.res, sizeof(double) * 6);
  if (n_warped) n_warped[i] = o.n_warped;
}

extern "C" int sdso_track_batch_prepare(sdso_ctx* ctx, int nprob, const int* ref_slots, const int* frame_slots, const sdso_track_eval_t* evs) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, nprob > 0 && ref_slots && frame_slots && evs, "bad batch arguments");
  std::vector<TrackProb> h(nprob);
  int maxn = 0;
  for (int i = 0; i < nprob; i++) {
    int rc = resolve_prob(ctx, ref_slots[i], frame_slots[i], evs[i], h[i]);
    if (rc) return rc;
    maxn = std::max(maxn, h[i].n);
  }
  int gx = choose_gx(ctx, nprob, maxn);
  int rc = batch_reserve(ctx, nprob, gx);
  if (rc) return rc;
  ctx->tb->nprob = nprob;
  ctx->tb->gx = gx;
  SDSO_HIP(ctx, hipMemcpy(ctx->tb->d_probs, h.data(), sizeof(TrackProb) * nprob, hipMemcpyHostToDevice));
  return SDSO_OK;
}

extern "C" int sdso_track_batch_enqueue(sdso_ctx* ctx) {
  if (!ctx || !ctx->tb || ctx->tb->nprob <= 0) return sdso::fail(ctx, SDSO_ERR_STATE, "no prepared batch");
  return launch_eval(ctx, ctx->tb->nprob, ctx->tb->gx, nullptr, true);
}

extern "C" int sdso_track_batch_fetch(sdso_ctx* ctx, double* H, double* b, double* res, int* n_warped) {
  if (!ctx || !ctx->tb || ctx->tb->nprob <= 0) return sdso::fail(ctx, SDSO_ERR_STATE, "no prepared batch");
  TrackBatch* tb = ctx->tb;
  int rc = ensure_pinned(ctx, sizeof(TrackOut) * tb->nprob);
  if (rc) return rc;
  SDSO_HIP(ctx, hipMemcpyAsync(ctx->pinned, tb->d_out, sizeof(TrackOut) * tb->nprob, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const TrackOut* o = (const TrackOut*)ctx->pinned;
  for (int i = 0; i < tb->nprob; i++) copy_out(o[i], i, H, b, res, n_warped);
  return SDSO_OK;
}

extern "C" int sdso_track_calc_res_gs_batch(sdso_ctx* ctx, int nprob, const int* ref_slots, const int* frame_slots,
                                            const sdso_track_eval_t* evs, double* H, double* b, double* res, int* n_warped) {
  int rc = sdso_track_batch_prepare(ctx, nprob, ref_slots, frame_slots, evs);
  if (rc) return rc;
  rc = sdso_track_batch_enqueue(ctx);
  if (rc) return rc;
  return sdso_track_batch_fetch(ctx, H, b, res, n_warped);
}

extern "C" int sdso_track_calc_res_gs(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_eval_t* ev, double* H, double* b,
                                      double* res, int* n_warped, uint8_t* inlier_mask) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, ev, "null eval");
  TrackProb P;
  int rc = resolve_prob(ctx, ref_slot, frame_slot, *ev, P);
  if (rc) return rc;
  rc = eval_now(ctx, &P, 1, inlier_mask);
  if (rc) return rc;
  copy_out(*(const TrackOut*)ctx->pinned, 0, H, b, res, n_warped);
  return SDSO_OK;
}
