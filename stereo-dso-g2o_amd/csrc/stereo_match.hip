// ------------------------------------------------------------------ left-right-left matching (S4)
// The callers of traceStereo all run the same three steps per point (FullSystem::stereoMatch FullSystem.cpp:581-613,
// traceNewCoarseNonKey :667-725, CoarseTracker::makeCoarseDepthL0 CoarseTracker.cpp:295-347):
//   ImmaturePoint(u, v, frameA) -> traceStereo(frameB)                       [forward]
//   if GOOD: ImmaturePoint(lastTraceUV, frameB) -> traceStereo(frameA)        [back]
// and then compare u with the back trace's lastTraceUV(0).  Everything stays on the device between the steps.
__global__ __launch_bounds__(256) void k_match_prepare(int n, const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ imin,
                                                       const float* __restrict__ imax, TraceDev T) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  fresh_point(T, p, u[p], v[p], 0.f, imin ? imin[p] : 0.f, imax ? imax[p] : NAN);
}
// back points at the forward trace's lastTraceUV; points whose forward trace was not GOOD are skipped (and parked on a
// harmless pixel so that the constructor kernel reads valid memory)
__global__ __launch_bounds__(256) void k_match_back_points(int n, TraceDev F, TraceDev Bk, uint8_t* __restrict__ skip, const float* __restrict__ bmin,
                                                           const float* __restrict__ bmax) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const bool good = F.status[p] == IPS_GOOD;
  skip[p] = good ? 0 : 1;
  fresh_point(Bk, p, good ? F.lastTraceUV[2 * p] : kTraceParkedPixel, good ? F.lastTraceUV[2 * p + 1] : kTraceParkedPixel, 0.f, bmin ? bmin[p] : 0.f, bmax ? bmax[p] : NAN);
}

namespace sdso {
// The launch sequence of a trace of fresh points, for stereo_match_chain_dev below and sdso_imm_trace (imm_trace.hip), each around its own
// prepare / back / accept kernels and on its own two batches.
// trace_pair_bind: F and Bk reserved and bound for n points, F's points lying on pyramid PA and searched in PB, Bk's on PB and searched in PA.
static int trace_pair_bind(sdso_ctx* ctx, TraceBatch& F, TraceBatch& Bk, int n, PyramidDev& PA, PyramidDev& PB, const float K[4], float baseline,
                           int mode_right_fwd, int mode_right_back) {
  for (TraceBatch* B : {&F, &Bk}) {
    SDSO_TRY(trace_reserve(ctx, *B, n));
    trace_bind(*B, n);
  }
  const int rc = trace_set_camera(ctx, F.T, PB, K, baseline, mode_right_fwd);
  return rc ? rc : trace_set_camera(ctx, Bk.T, PA, K, baseline, mode_right_back);
}
// launch_fresh_trace: ImmaturePoint::ImmaturePoint on `host` for the points of T, then their traceStereo; skip[p] = 1 leaves point p alone.
// (k_trace_stereo is timed at profiling level 1 — a chain's two traces —, k_immature_init at level 2.)
static void launch_fresh_trace(sdso_ctx* ctx, TraceDev T, const PyramidDev& host, const uint8_t* skip) {
  launch_timed(ctx, "k_immature_init", 2, k_immature_init, dim3((T.n + 255) / 256), dim3(256), (const float4*)host.d[0], T.w, T.n, (const float*)T.u_stereo,
               (const float*)T.v_stereo, (float*)T.color, (float*)T.weights, (float*)T.gradH, (float*)T.energyTH);
  T.skip = skip;
  launch_trace_stereo(ctx, T);
}

// The chain on device-resident inputs: in[0..5] = u, v, idepth_min_stereo, idepth_max_stereo, and the back trace's two bounds (each n
// floats in device memory; 2..5 may be null: 0 / NaN, a fresh ImmaturePoint), skip_fwd (optional, n bytes): 1 = the point takes no trace
// at all (both statuses 255; its u, v must still address a readable pattern).  Enqueue only: the results stay in the ctx's two match
// batches (*out points into them) until the next chain of this ctx.  The caller has validated the slots.
int stereo_match_chain_dev(sdso_ctx* ctx, int slot_a, int slot_b, const float K[4], float baseline, int mode_right_first, int n,
                           const float* const in[6], const uint8_t* skip_fwd, MatchChainOut* out) {
  PyramidDev& PA = ctx->pyr.find(slot_a)->second;
  PyramidDev& PB = ctx->pyr.find(slot_b)->second;
  StereoState& S = stereo_state(ctx);
  TraceBatch& A = S.match[0];    // forward: points of frame A searched in frame B
  TraceBatch& Bk = S.match[1];   // back: points of frame B searched in frame A
  SDSO_TRY(trace_pair_bind(ctx, A, Bk, n, PA, PB, K, baseline, mode_right_first ? 1 : 0, mode_right_first ? 0 : 1));
  const dim3 g1((n + 255) / 256), b1(256);
  uint8_t* skip = Bk.skip();
  hipLaunchKernelGGL(k_match_prepare, g1, b1, 0, ctx->stream, n, in[0], in[1], in[2], in[3], A.T);
  launch_fresh_trace(ctx, A.T, PA, skip_fwd);
  hipLaunchKernelGGL(k_match_back_points, g1, b1, 0, ctx->stream, n, A.T, Bk.T, skip, in[4], in[5]);
  launch_fresh_trace(ctx, Bk.T, PB, skip);
  SDSO_HIP(ctx, hipGetLastError());
  out->idepth_stereo = A.T.idepth_stereo; out->idepth_min = A.T.idepth_min_stereo; out->idepth_max = A.T.idepth_max_stereo;
  out->fwd_uv = A.T.lastTraceUV; out->back_uv = Bk.T.lastTraceUV; out->status_fwd = A.T.status; out->status_back = Bk.T.status;
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_stereo_match_batch(sdso_ctx* ctx, int slot_a, int slot_b, const float K[4], float baseline, int mode_right_first,
                                       sdso_stereo_match_t* M) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, K && M && M->n >= 0, "null argument");
  PyramidDev *PA = nullptr, *PB = nullptr;
  SDSO_TRY(frame_pyramid(ctx, slot_a, &PA));
  SDSO_TRY(frame_pyramid_sized(ctx, slot_b, PA->w[0], PA->h[0], "the two frames differ in size", &PB));
  const int n = M->n, w = PA->w[0], h = PA->h[0];
  if (n == 0) return SDSO_OK;
  SDSO_REQUIRE(ctx, M->u && M->v, "null point arrays");
  for (int i = 0; i < n; i++)
    SDSO_REQUIRE(ctx, trace_pattern_readable(M->u[i], M->v[i], w, h), "immature point too close to the image border");
  // host inputs -> device
  const float* d_in[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const float* h_in[6] = {M->u, M->v, M->idepth_min_stereo, M->idepth_max_stereo, M->back_idepth_min_stereo, M->back_idepth_max_stereo};
  SDSO_TRY(ensure_scratch(ctx, sizeof(float) * 6 * (size_t)n));
  for (int k = 0; k < 6; k++)
    if (h_in[k]) {
      float* d = (float*)ctx->scratch + (size_t)k * n;
      SDSO_HIP(ctx, hipMemcpyAsync(d, h_in[k], sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
      d_in[k] = d;
    }
  MatchChainOut o;
  SDSO_TRY(stereo_match_chain_dev(ctx, slot_a, slot_b, K, baseline, mode_right_first, n, d_in, nullptr, &o));
  const struct { float* dst; const float* src; int width; } outs[] = {{M->idepth_stereo, o.idepth_stereo, 1}, {M->idepth_min_out, o.idepth_min, 1},
                                                                     {M->idepth_max_out, o.idepth_max, 1}, {M->fwd_uv, o.fwd_uv, 2}, {M->back_uv, o.back_uv, 2}};
  for (const auto& c : outs)
    if (c.dst) SDSO_HIP(ctx, hipMemcpyAsync(c.dst, c.src, sizeof(float) * (size_t)c.width * n, hipMemcpyDeviceToHost, ctx->stream));
  if (M->status_fwd) SDSO_HIP(ctx, hipMemcpyAsync(M->status_fwd, o.status_fwd, n, hipMemcpyDeviceToHost, ctx->stream));
  if (M->status_back) SDSO_HIP(ctx, hipMemcpyAsync(M->status_back, o.status_back, n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}
