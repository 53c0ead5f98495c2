// The fork-live coarse tracker resident on the device (part of g2o_factors.hip): k_g2o_track_lm runs whole tries of
// CoarseTracker::trackNewestCoarse (CoarseTracker.cpp:827-1069) — every calcRes, every linearisation, g2o's Levenberg-Marquardt around
// them — in ONE launch, one workgroup per try, and records each try's event trace; on top of it sdso_g2o_track_newest_coarse_batch and
// sdso_g2o_track_new_coarse, the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511) with the fork-live body.
//
// Who does what.  The try is g2o_track::Core (g2o_track_core.h), the text sdso_g2o_track_newest_coarse has on the host, cut at its
// evaluations.  Per evaluation all lanes of the workgroup stride over the level's points with the edge bodies of g2o_factors.hip
// (track_cull, track_edge<JAC>, track_lin_add), the sums go through a wave butterfly into one LDS row per wave and are folded in wave
// order, and thread 0 takes the controller's step between two barriers: solve, exp, accept or reject, the next request.  The evaluation
// record stays in LDS.  Nothing is read that another workgroup writes: no flag, no spin, no wait across workgroups, and every loop is
// bounded by constants (kMaxEvaluations, strided point loops) — the kernel ends by construction.
// The try's edge mask is private to the try (a work buffer of sum pc_n bytes); the Xref of an edge is recomputed from its pc point (three
// float divisions).  The edge sets of sdso_g2o_track_add_edges (ctx->g2o->sets) are not touched.
// Determinism: a lane's points, the butterfly and the fold order depend on the level size alone — reruns are bit-identical and a try's
// result does not depend on the size of the batch or its place in it.
namespace sdso {

constexpr int GT_BLOCK = 512;              // 8 waves, two per SIMD: the 46 f64 sums of a lane alone are 92 VGPRs
constexpr int GT_WAVES = GT_BLOCK / 64;
constexpr int GT_LEVELS = 5;               // trackNewestCoarse walks at most five levels (the assert of :853)

struct G2oTrackJob {
  sdso_track_params_t p;
  sdso_se3_t T;                            // in: lastToNew; out where the try reached STEP4 (:1044-1045)
  sdso_aff_t aff;
  const float4* pc[GT_LEVELS];
  const float4* img[GT_LEVELS];
  int n[GT_LEVELS];
  int mask_off[GT_LEVELS];                 // the level's part of `mask`
  sdso_g2o_track_eval_t base[GT_LEVELS];   // the level's constants: camera, Ki, the cull tables at the call's initial pose, thresholds
  uint8_t* mask;                           // sum of n[] bytes, the try's own
  float* flow;                             // 4 floats per 32nd level-0 point, the try's own
  sdso_track_result_t out;
  sdso_track_trace_t trace;
  int finished;
};

// one edge into a lane's {chi2, robust chi2}: the two sums of track_lin_add that computeActiveErrors alone gives
__device__ __forceinline__ void track_chi_add(double e, double delta, double& s_e2, double& s_rho0) {
  const double e2 = e * e, dsqr = delta * delta;
  double rho0;
  if (e2 <= dsqr) rho0 = e2;
  else { const double sqrte = sqrt(e2); rho0 = 2 * sqrte * delta - dsqr; }
  s_e2 += e2;
  s_rho0 += rho0;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the request out of LDS into scalar registers, dword by dword: it is the same in every lane, and as vector registers next to a lane's 46
// f64 sums it would not fit the 256 a wave of this workgroup has
__device__ __forceinline__ sdso_g2o_track_eval_t track_eval_uniform(const sdso_g2o_track_eval_t& src) {
  static_assert(sizeof(sdso_g2o_track_eval_t) % 4 == 0, "whole dwords");
  sdso_g2o_track_eval_t dst;
  const int* s = reinterpret_cast<const int*>(&src);
  int* d = reinterpret_cast<int*>(&dst);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(sdso_g2o_track_eval_t) / 4); k++) d[k] = __builtin_amdgcn_readfirstlane(s[k]);
  return dst;
}

__global__ __launch_bounds__(GT_BLOCK) void k_g2o_track_lm(G2oTrackJob* __restrict__ jobs, int nhyp) {
  const int c = blockIdx.x;
  if (c >= nhyp) return;
  G2oTrackJob& J = jobs[c];
  __shared__ __align__(16) unsigned char core_raw[sizeof(g2o_track::Core)];   // (Se3 has member initialisers: raw storage, init() sets every field)
  g2o_track::Core& core = *reinterpret_cast<g2o_track::Core*>(core_raw);
  __shared__ sdso_g2o_track_eval_t ev;     // the pending request
  __shared__ g2o_track::Eval E;            // its evaluation
  __shared__ double sW[GT_WAVES][kSysDoubles];
  __shared__ int s_cnt[2];                 // {numTermsInE, numSaturated}
  __shared__ double s_work[80];            // solveLdltSmall's storage
  __shared__ int s_piv[8];
  __shared__ int s_req, s_lvl, s_done;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    core.init(J.p, J.n, J.T, J.aff);
    ev = J.base[core.lvl];
    g2o_track::fill_request(core, ev);
    s_req = core.req; s_lvl = core.lvl; s_done = 0;
    s_cnt[0] = 0; s_cnt[1] = 0;
  }
  __syncthreads();
  for (int e = 0; e < g2o_track::kMaxEvaluations; e++) {
    const int req = __builtin_amdgcn_readfirstlane(s_req), lvl = __builtin_amdgcn_readfirstlane(s_lvl);
    const int n = J.n[lvl];
    const sdso_g2o_track_eval_t evu = track_eval_uniform(ev);
    const float4* __restrict__ pc = J.pc[lvl];
    const float4* __restrict__ img = J.img[lvl];
    uint8_t* __restrict__ mask = J.mask + J.mask_off[lvl];
    if (req == g2o_track::REQ_CALCRES) {                      // calcRes: the cull, the edges, the saturation test
      int term = 0, sat = 0;
      for (int i = tid; i < n; i += GT_BLOCK) {
        float4 xr;
        int s1;
        const uint8_t m = track_cull(pc[i], img, evu, xr, s1, lvl == 0 && i % 32 == 0 ? J.flow + (size_t)(i / 32) * 4 : nullptr);
        mask[i] = m;
        term += m; sat += s1;
      }
      term = wave_sum_int(term); sat = wave_sum_int(sat);
      if (lane == 0) {
        if (term) atomicAdd(&s_cnt[0], term);
        if (sat) atomicAdd(&s_cnt[1], sat);
      }
    } else if (req == g2o_track::REQ_LINEARIZE) {             // computeActiveErrors + linearizeOplus + the quadratic form
      double acc[kSysDoubles];
#pragma unroll
      for (int k = 0; k < kSysDoubles; k++) acc[k] = 0;
      for (int i = tid; i < n; i += GT_BLOCK) {
        if (!mask[i]) continue;
        const TrackEdgeVal v = track_edge<true>(track_xref(pc[i], evu), img, evu);
        track_lin_add(v, evu.huberTH, acc);
      }
#pragma unroll
      for (int k = 0; k < kSysDoubles; k++) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) sW[wv][k] = s;
      }
    } else {                                                  // computeActiveErrors alone
      double s_e2 = 0, s_rho0 = 0;
      for (int i = tid; i < n; i += GT_BLOCK) {
        if (!mask[i]) continue;
        const TrackEdgeVal v = track_edge<false>(track_xref(pc[i], evu), img, evu);
        track_chi_add(v.e, evu.huberTH, s_e2, s_rho0);
      }
      s_e2 = wave_sum(s_e2); s_rho0 = wave_sum(s_rho0);
      if (lane == 0) { sW[wv][44] = s_e2; sW[wv][45] = s_rho0; }
    }
    __syncthreads();
    if (tid < kSysDoubles && (req == g2o_track::REQ_LINEARIZE || (req == g2o_track::REQ_ERRORS && tid >= 44))) {   // the fold, in wave order
      double s = sW[0][tid];
#pragma unroll
      for (int w = 1; w < GT_WAVES; w++) s += sW[w][tid];
      E.sums[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {                                           // the serial part: the controller's step and the next request
      if (req == g2o_track::REQ_CALCRES) {
        E.n_edges = s_cnt[0]; E.n_saturated = s_cnt[1];
        s_cnt[0] = 0; s_cnt[1] = 0;
        float sT = 0, sRT = 0, sN = 0;                        // :662-693 in point order, the loop of sdso_g2o_track_add_edges
        if (lvl == 0) {
          const int nflow = (n + 31) / 32;
          const float4* __restrict__ f = reinterpret_cast<const float4*>(J.flow);
#pragma unroll 8
          for (int k = 0; k < nflow; k++) { const float4 q = f[k]; sT += q.x; sT += q.y; sRT += q.z; sRT += q.w; sN += 2; }
        }
        E.flow[0] = sT / (sN + 0.1);
        E.flow[1] = 0;
        E.flow[2] = sRT / (sN + 0.1);
      }
      core.consume(E, s_work, s_piv);
      if (core.done) s_done = 1;
      else {
        if (core.lvl != lvl) ev = J.base[core.lvl];
        g2o_track::fill_request(core, ev);
        s_req = core.req; s_lvl = core.lvl;
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  if (tid == 0) {
    // member by member into the job the host zeroed: the bytes that come back are a function of the values alone (no padding out of LDS)
    J.out.good = core.out.good; J.out.evaluations = core.out.evaluations; J.out.point_evals = core.out.point_evals;
    for (int i = 0; i < 5; i++) { J.out.lastResiduals[i] = core.out.lastResiduals[i]; J.out.iterations[i] = core.out.iterations[i]; }
    for (int i = 0; i < 3; i++) J.out.lastFlowIndicators[i] = core.out.lastFlowIndicators[i];
    J.trace.n = core.trace.n;
    for (int e = 0; e < SDSO_TRACK_MAX_EVENTS; e++) {
      J.trace.lvl[e] = core.trace.lvl[e]; J.trace.res[e] = core.trace.res[e];
      for (int k = 0; k < 3; k++) J.trace.flow[e][k] = core.trace.flow[e][k];
    }
    if (core.wrote_final) { J.T = core.T_final; J.aff = core.aff_final; }
    J.finished = s_done;
  }
}

// nhyp tries in one launch; the contract of track_newest_coarse_run (tracker_lm_api.hip): lastToNew / aff_g2l in/out like the single
// call's references, traces (may be null) the event trace of every try.  Every refusal comes before any device work.
static int g2o_track_newest_coarse_run(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                       sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs, sdso_track_trace_t* traces) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, nhyp > 0 && ref_slots && frame_slots && prms && lastToNew && aff_g2l && outs, "null argument");
  for (int k = 0; k < nhyp; k++) SDSO_TRY(track_coarsest_level_ok(ctx, prms[k]));
  std::vector<G2oTrackJob> jobs((size_t)nhyp);
  std::vector<size_t> mask_at((size_t)nhyp), flow_at((size_t)nhyp);
  size_t mask_total = 0, flow_total = 0;
  for (int k = 0; k < nhyp; k++) {
    G2oTrackJob& J = jobs[k];
    std::memset(&J, 0, sizeof(J));
    const sdso_track_params_t& p = prms[k];
    J.p = p; J.T = lastToNew[k]; J.aff = aff_g2l[k];
    int off = 0;
    for (int l = 0; l <= p.coarsestLvl; l++) {
      TrackLevel TL;
      SDSO_TRY(track_level(ctx, ref_slots[k], frame_slots[k], l, p.w[l], p.h[l], &TL));
      J.pc[l] = TL.pc; J.img[l] = TL.img; J.n[l] = TL.n; J.mask_off[l] = off;
      off += (TL.n + 15) & ~15;
      sdso_track_eval_t base;                                 // as sdso_g2o_track_newest_coarse derives its records
      sdso_track_make_eval(&p, l, &lastToNew[k], &aff_g2l[k], 1.0f, &base);
      sdso_g2o_track_eval_t& ev = J.base[l];
      ev.lvl = l; ev.w = base.w; ev.h = base.h; ev.fx = base.fx; ev.fy = base.fy; ev.cx = base.cx; ev.cy = base.cy;
      std::memcpy(ev.Ki, base.Ki, sizeof(ev.Ki)); std::memcpy(ev.RKi, base.RKi, sizeof(ev.RKi)); std::memcpy(ev.t_cull, base.t, sizeof(ev.t_cull));
      std::memcpy(ev.R, lastToNew[k].R, sizeof(ev.R)); std::memcpy(ev.t, lastToNew[k].t, sizeof(ev.t));
      ev.ab[0] = base.affLL[0]; ev.ab[1] = base.affLL[1];
      ev.b0 = p.ref_aff_g2l.b;
      ev.cutoffTH = base.cutoffTH; ev.huberTH = base.huberTH;
    }
    mask_at[k] = mask_total; mask_total += (size_t)off + 16;
    flow_at[k] = flow_total; flow_total += 4 * ((size_t)(J.n[0] + 31) / 32) + 4;
  }
  if (!ctx->g2o) ctx->g2o = new G2oState();
  G2oState& st = *ctx->g2o;
  const size_t jobs_bytes = sizeof(G2oTrackJob) * (size_t)nhyp;
  SDSO_HIP(ctx, st.lm_jobs_host.reserve(ctx->stream, jobs_bytes, sizeof(G2oTrackJob) * (size_t)std::max(nhyp, 8)));
  SDSO_HIP(ctx, st.lm_jobs.reserve(ctx->stream, jobs_bytes, sizeof(G2oTrackJob) * (size_t)std::max(nhyp, 8)));
  SDSO_HIP(ctx, st.lm_mask.reserve(ctx->stream, mask_total, mask_total + mask_total / 4 + 4096));
  SDSO_HIP(ctx, st.lm_flow.reserve(ctx->stream, flow_total, flow_total + flow_total / 4 + 1024));
  for (int k = 0; k < nhyp; k++) { jobs[k].mask = st.lm_mask.get() + mask_at[k]; jobs[k].flow = st.lm_flow.get() + flow_at[k]; }
  G2oTrackJob* hj = (G2oTrackJob*)st.lm_jobs_host;
  G2oTrackJob* dj = (G2oTrackJob*)st.lm_jobs;
  std::memcpy(hj, jobs.data(), jobs_bytes);
  SDSO_HIP(ctx, hipMemcpyAsync(dj, hj, jobs_bytes, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "k_g2o_track_lm");
    hipLaunchKernelGGL(k_g2o_track_lm, dim3(nhyp), dim3(GT_BLOCK), 0, ctx->stream, dj, nhyp);
  }
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipMemcpyAsync(hj, dj, jobs_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < nhyp; k++)
    if (!hj[k].finished) return fail(ctx, SDSO_ERR_STATE, "k_g2o_track_lm: a try did not end within its bound of evaluations");   // (cannot happen)
  for (int k = 0; k < nhyp; k++) { outs[k] = hj[k].out; lastToNew[k] = hj[k].T; aff_g2l[k] = hj[k].aff; }
  if (traces) for (int k = 0; k < nhyp; k++) traces[k] = hj[k].trace;
  return SDSO_OK;
}

}  // namespace sdso

extern "C" int sdso_g2o_track_newest_coarse_batch(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                                  sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs) {
  return g2o_track_newest_coarse_run(ctx, nhyp, ref_slots, frame_slots, prms, lastToNew, aff_g2l, outs, nullptr);
}

extern "C" int sdso_g2o_track_new_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries,
                                         const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold,
                                         sdso_track_tries_result_t* out, sdso_track_try_t* recs) {
  return track_new_coarse_with(ctx, ref_slot, frame_slot, prm, ntries, tries, aff_last_2_l, lastCoarseRMSE, reTrackThreshold, out, recs,
                               g2o_track_newest_coarse_run);
}
