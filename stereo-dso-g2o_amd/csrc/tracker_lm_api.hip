// trackNewestCoarse through the C-ABI: the jobs of the resident driver k_track_lm, the lock-step host driver, the entry points (part of tracker.hip).
namespace sdso {
static int resolve_job(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t& p, LmJob& J) {
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) { J.pc[l] = nullptr; J.img[l] = nullptr; J.n[l] = 0; }
  for (int l = 0; l <= p.coarsestLvl; l++) {
    TrackLevel L;
    int rc = track_level(ctx, ref_slot, frame_slot, l, p.w[l], p.h[l], &L);
    if (rc) return rc;
    J.pc[l] = L.pc; J.img[l] = L.img; J.n[l] = L.n;
  }
  J.p = p;
  return SDSO_OK;
}
}  // namespace sdso

// the lock-step host driver (A/B and fallback for SDSO_TRK_HOST_LM=1)
static int track_newest_coarse_host(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                    sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs, sdso_track_trace_t* traces) {
  std::vector<LmCore> S(nhyp);
  for (int k = 0; k < nhyp; k++) S[k].init(prms[k], lastToNew[k], aff_g2l[k]);
  std::vector<TrackProb> probs;
  std::vector<int> who;
  for (;;) {
    probs.clear(); who.clear();
    for (int k = 0; k < nhyp; k++) {
      LmCore& s = S[k];
      if (s.done) continue;
      sdso_track_eval_t ev;
      fill_eval(s.p, s.lvl, s.reqT, s.reqAff, s.p.coarseCutoffTH * s.levelCutoffRepeat, ev);
      TrackProb P;
      int rc = resolve_prob(ctx, ref_slots[k], frame_slots[k], ev, P);
      if (rc) return rc;
      probs.push_back(P); who.push_back(k);
      s.out.evaluations++;
      s.out.point_evals += P.n;
    }
    if (probs.empty()) break;
    int rc = eval_now(ctx, probs.data(), (int)probs.size(), nullptr);
    if (rc) return rc;
    const TrackOut* O = (const TrackOut*)ctx->pinned;
    for (size_t j = 0; j < who.size(); j++) S[who[j]].consume(O[j]);
  }
  for (int k = 0; k < nhyp; k++) {
    outs[k] = S[k].out;
    if (traces) traces[k] = S[k].trace;
    if (S[k].wrote_final) { lastToNew[k] = S[k].T_final; aff_g2l[k] = S[k].aff_final; }
  }
  return SDSO_OK;
}

// sdso_track_newest_coarse_batch; traces (may be null): the event trace of every hypothesis, for sdso_track_new_coarse (tracker_tries.hip)
static int track_newest_coarse_run(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                   sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs, sdso_track_trace_t* traces) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, nhyp > 0 && ref_slots && frame_slots && prms && lastToNew && aff_g2l && outs, "null argument");
  for (int k = 0; k < nhyp; k++) {
    int rc = track_coarsest_level_ok(ctx, prms[k]);
    if (rc) return rc;
  }
  static const bool host_lm = dbg_env("SDSO_TRK_HOST_LM") != nullptr;
  if (host_lm) return track_newest_coarse_host(ctx, nhyp, ref_slots, frame_slots, prms, lastToNew, aff_g2l, outs, traces);
  // resident driver: jobs through pinned memory, one launch, one synchronisation.  The cluster records are the library's own allocation
  // and are never cleared between calls (tags, see LmCluster).  (The kernel reading the jobs in pinned host memory directly, without
  // the two copies, measured the same 0.305 ms per call: tools/time_track.py, round 5.)
  int rc = ensure_pinned(ctx, sizeof(LmJob) * (size_t)nhyp);
  if (rc) return rc;
  const size_t jobs_bytes = (sizeof(LmJob) * (size_t)nhyp + 255) & ~(size_t)255;
  rc = ensure_scratch(ctx, jobs_bytes);
  if (rc) return rc;
  if (ctx->lm_clusters.cap() < sizeof(LmCluster) * (size_t)nhyp || ctx->lm_epoch > (1 << 30)) {
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SDSO_HIP(ctx, ctx->lm_clusters.reserve(ctx->stream, sizeof(LmCluster) * (size_t)nhyp, sizeof(LmCluster) * (size_t)std::max(nhyp, 8)));
    SDSO_HIP(ctx, hipMemsetAsync(ctx->lm_clusters, 0, ctx->lm_clusters.cap(), ctx->stream));
    ctx->lm_epoch = 0;
  }
  LmJob* hj = (LmJob*)ctx->pinned;
  for (int k = 0; k < nhyp; k++) {
    rc = resolve_job(ctx, ref_slots[k], frame_slots[k], prms[k], hj[k]);
    if (rc) return rc;
  }
  if (ctx->tb) ctx->tb->nprob = 0;   // (a prepared evaluation batch keeps its own buffers; nothing shared)
  LmJob* dj = (LmJob*)ctx->scratch;
  LmCluster* dc = (LmCluster*)ctx->lm_clusters;
  // workgroups per hypothesis: as many as keep the whole grid resident at once (the members of a cluster wait for each other; one
  // 512-thread workgroup of this kernel fills a CU), eight at most.  SDSO_TRK_LM_CLUSTER=1 forces single workgroups.
  const int g_env = dbg_env("SDSO_TRK_LM_CLUSTER") ? atoi(dbg_env("SDSO_TRK_LM_CLUSTER")) : 0;   // (read per call: the tests walk the cluster sizes)
  const int slots8 = 8 * ((nhyp + 7) / 8);
  int G = std::min(LM_MAXG, (ctx->n_cu * 7 / 8) / slots8);   // (an eighth of the CUs stays free: a grid that needs every CU waits on any straggler)
  if (g_env > 0) G = std::min(G, g_env);
  if (G < 2) G = 1;
  const int solo_n = dbg_env("SDSO_TRK_LM_SOLO") ? atoi(dbg_env("SDSO_TRK_LM_SOLO")) : LM_UNROLL * LM_BLOCK;
#ifdef SDSO_TEST_HOOKS
  // test hook, compiled into libsdso_hip_hooks.so only (csrc/Makefile; tests/test_variants_gpu.py): the first attempt loses one member of
  // every cluster, with a short spin limit — the call must come back through the single-workgroup repetition with its result
  const bool drop = dbg_env("SDSO_TRK_LM_TEST_DROP_MEMBER") != nullptr;
#else
  const bool drop = false;
#endif
  for (int attempt = 0; attempt < 2; attempt++) {
    for (int k = 0; k < nhyp; k++) { hj[k].T = lastToNew[k]; hj[k].aff = aff_g2l[k]; hj[k].out.evaluations = -1; }   // (-1 until member 0 reports)
    SDSO_HIP(ctx, hipMemcpyAsync(dj, hj, sizeof(LmJob) * nhyp, hipMemcpyHostToDevice, ctx->stream));
    const int e_base = ctx->lm_epoch;
    ctx->lm_epoch += 1040;             // (a call has at most 1024 evaluations)
    {
      ProfScope ps(ctx, "k_track_lm");
      hipLaunchKernelGGL(k_track_lm, dim3(G > 1 ? slots8 * G : nhyp), dim3(LM_BLOCK), 0, ctx->stream, dj, dc, nhyp, G, drop ? 1 << 12 : LM_SPIN_LIMIT, drop && G > 1 ? 1 : 0, solo_n, e_base);
    }
    SDSO_HIP(ctx, hipGetLastError());
    SDSO_HIP(ctx, hipMemcpyAsync(hj, dj, sizeof(LmJob) * nhyp, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    bool gave_up = false;
    for (int k = 0; k < nhyp; k++) gave_up = gave_up || hj[k].out.evaluations < 0;
    if (!gave_up) break;
    SDSO_REQUIRE(ctx, G > 1, "k_track_lm gave up without a cluster");   // (cannot happen: single workgroups wait for nobody)
    G = 1;                             // a cluster was not co-resident (shared device): the single-workgroup form needs no co-residency
  }
  for (int k = 0; k < nhyp; k++) { outs[k] = hj[k].out; lastToNew[k] = hj[k].T; aff_g2l[k] = hj[k].aff; }
  if (traces) for (int k = 0; k < nhyp; k++) traces[k] = hj[k].trace;
  return SDSO_OK;
}

extern "C" int sdso_track_newest_coarse_batch(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                              sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs) {
  return track_newest_coarse_run(ctx, nhyp, ref_slots, frame_slots, prms, lastToNew, aff_g2l, outs, nullptr);
}

extern "C" int sdso_track_newest_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm,
                                        sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, prm && lastToNew && aff_g2l && out, "null argument");
  return sdso_track_newest_coarse_batch(ctx, 1, &ref_slot, &frame_slot, prm, lastToNew, aff_g2l, out);
}
