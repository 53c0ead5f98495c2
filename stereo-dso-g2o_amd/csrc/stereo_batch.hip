// TraceBatch: the device-resident point arrays of one trace, its members and private areas stated once; the ctx's StereoState; the
// host-buffer entry points around the kernels of stereo_trace.hip.
namespace sdso {
// ---- the members: one blob of kTbFloats * n floats, structure of arrays with stride n (TB_* = offsets in units of n floats), and
// kTbBytes * n bytes.  The in/out fields {idepth_min_stereo, idepth_max_stereo, quality, idepth_stereo} are contiguous, with a pristine
// copy at TB_PRISTINE, so that enqueue can be repeated on identical input (benchmark).  idepth_stereo is written only for GOOD points
// (ImmaturePoint.cpp:448): without its copy, an enqueue in another refinement mode would return the previous enqueue's value for a
// point that was GOOD there and is not now.
enum { TB_U = 0, TB_V = 1, TB_IMIN = 2, TB_IMIN_S = 3, TB_IMAX_S = 4, TB_QUAL = 5, TB_IDEPTH_S = 6, TB_COLOR = 7, TB_WEIGHTS = 15, TB_GRADH = 23, TB_ETH = 27,
       TB_UV = 28, TB_INTERVAL = 30, TB_PRISTINE = 32 };
constexpr int kTbInOut = TB_IMIN_S, kTbInOutWidth = 4, kTbFloats = 36, kTbBytes = 3;   // bytes: lastTraceStatus | status | pristine lastTraceStatus
using TracePts = sdso_trace_points_t;
struct TbMember { float* TracePts::*host; int off, width; bool fetched; };   // the caller's array; fetched: an output of the trace
constexpr TbMember kTbMembers[] = {
    {&TracePts::u_stereo, TB_U, 1, false},     {&TracePts::v_stereo, TB_V, 1, false},       {&TracePts::idepth_min, TB_IMIN, 1, false},
    {&TracePts::idepth_min_stereo, TB_IMIN_S, 1, true},  {&TracePts::idepth_max_stereo, TB_IMAX_S, 1, true},  {&TracePts::quality, TB_QUAL, 1, true},
    {&TracePts::idepth_stereo, TB_IDEPTH_S, 1, true},    {&TracePts::color, TB_COLOR, 8, false},    {&TracePts::weights, TB_WEIGHTS, 8, false},
    {&TracePts::gradH, TB_GRADH, 4, false},    {&TracePts::energyTH, TB_ETH, 1, false},     {&TracePts::lastTraceUV, TB_UV, 2, true},
    {&TracePts::lastTracePixelInterval, TB_INTERVAL, 1, true}};
constexpr int tb_members_end() {   // the first float past the last member, or -1 where a member does not start at its predecessor's end
  int o = 0;
  for (const TbMember& m : kTbMembers) { if (m.off != o) return -1; o += m.width; }
  return o;
}
static_assert(tb_members_end() > 0 && tb_members_end() <= TB_PRISTINE && TB_PRISTINE + kTbInOutWidth == kTbFloats,
              "the members in order, then the pristine copy of the in/out fields, fill the kTbFloats columns trace_reserve allocates");
static_assert(kTbMembers[3].off == kTbInOut && kTbMembers[6].off + kTbMembers[6].width == kTbInOut + kTbInOutWidth, "the in/out fields are one run of columns");

// device-resident batch used by both the host-buffer entry point and the benchmark
struct TraceBatch {
  TraceDev T;
  DevBuf<float> blob;      // all float arrays
  DevBuf<uint8_t> bytes;
  int n = 0;               // the stride: points reserved, >= T.n
  float* col(int c) const { return blob + (size_t)c * n; }
  // the private areas, which no TraceDev member names
  float* inout() const { return col(kTbInOut); }
  float* pristine() const { return col(TB_PRISTINE); }
  uint8_t* pristine_status() const { return bytes + 2 * (size_t)n; }
  // A batch of a chain (stereo_match_chain_dev, sdso_imm_trace) is written anew by every chain and never enqueued twice: it has no
  // pristine copy, and the chain borrows those areas for its skip bytes and for the projected interval of its points.
  uint8_t* skip() const { return pristine_status(); }
  float* pmin() const { return pristine(); }
  float* pmax() const { return pristine() + n; }
};
struct StereoState {
  TraceBatch* trace = nullptr;   // the prepared traceStereo batch (sdso_trace_stereo_prepare / _enqueue / _fetch)
  TraceBatch match[2];           // forward and back batches of sdso_stereo_match_batch
};
static StereoState& stereo_state(sdso_ctx* ctx) { if (!ctx->stereo) ctx->stereo = new StereoState(); return *ctx->stereo; }
static TraceBatch* prepared_trace(sdso_ctx* ctx) { return ctx && ctx->stereo ? ctx->stereo->trace : nullptr; }

static int trace_reserve(sdso_ctx* ctx, TraceBatch& B, int n) {
  if (B.n >= n) return SDSO_OK;
  const size_t cap = (size_t)(n + n / 4 + 64);
  B.n = 0;   // a group (devbuf.h)
  SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, B.blob, B.bytes));
  SDSO_HIP(ctx, B.blob.reserve(ctx->stream, cap * kTbFloats, cap * kTbFloats));
  SDSO_HIP(ctx, B.bytes.reserve(ctx->stream, cap * kTbBytes, cap * kTbBytes));
  B.n = (int)cap;
  return SDSO_OK;
}
static void trace_bind(TraceBatch& B, int n) {
  TraceDev& T = B.T;
  T.n = n;
  T.u_stereo = B.col(TB_U); T.v_stereo = B.col(TB_V); T.idepth_min = B.col(TB_IMIN); T.idepth_min_stereo = B.col(TB_IMIN_S);
  T.idepth_max_stereo = B.col(TB_IMAX_S); T.quality = B.col(TB_QUAL); T.idepth_stereo = B.col(TB_IDEPTH_S); T.color = B.col(TB_COLOR);
  T.weights = B.col(TB_WEIGHTS); T.gradH = B.col(TB_GRADH); T.energyTH = B.col(TB_ETH); T.lastTraceUV = B.col(TB_UV);
  T.lastTracePixelInterval = B.col(TB_INTERVAL);
  T.lastTraceStatus = B.bytes; T.status = B.bytes + (size_t)B.n; T.skip = nullptr;
}
// where and how the points of T are searched: level 0 of P (its intensity plane built), the camera, the side
static int trace_set_camera(sdso_ctx* ctx, TraceDev& T, PyramidDev& P, const float K[4], float baseline, int mode_right) {
  SDSO_TRY(ensure_plane0(ctx, P));
  T.w = P.w[0]; T.h = P.h[0]; T.mode_right = mode_right; T.img = P.d[0]; T.plane = P.plane0;
  T.fx = K[0]; T.fy = K[1]; T.cx = K[2]; T.cy = K[3]; T.baseline = baseline;
  return SDSO_OK;
}
void release_stereo(sdso_ctx* ctx) {
  if (ctx->stereo) delete ctx->stereo->trace;
  delete ctx->stereo;
  ctx->stereo = nullptr;
}
}  // namespace sdso

extern "C" int sdso_immature_init_batch(sdso_ctx* ctx, int frame_slot, int n, const float* u, const float* v, float* color, float* weights,
                                        float* gradH, float* energyTH) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  PyramidDev* P = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &P));
  SDSO_REQUIRE(ctx, n >= 0 && (n == 0 || (u && v && color && weights && gradH && energyTH)), "null argument");
  if (n == 0) return SDSO_OK;
  const int w = P->w[0], h = P->h[0];
  for (int i = 0; i < n; i++)  // the reference dereferences the 3x3 neighbourhood unchecked; refuse instead of faulting
    SDSO_REQUIRE(ctx, trace_pattern_readable(u[i], v[i], w, h), "immature point too close to the image border");
  SDSO_TRY(ensure_scratch(ctx, sizeof(float) * (size_t)n * 23));
  float* d = (float*)ctx->scratch;
  float *du = d, *dv = d + n, *dc = d + 2 * (size_t)n, *dw = d + 10 * (size_t)n, *dg = d + 18 * (size_t)n, *de = d + 22 * (size_t)n;
  SDSO_HIP(ctx, hipMemcpyAsync(du, u, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(dv, v, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_immature_init, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, P->d[0], w, n, du, dv, dc, dw, dg, de);
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipMemcpyAsync(color, dc, sizeof(float) * 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(weights, dw, sizeof(float) * 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(gradH, dg, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(energyTH, de, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

// upload the point state once (benchmark: state stays in HBM, enqueue-only launches follow)
extern "C" int sdso_trace_stereo_prepare(sdso_ctx* ctx, int frame_slot, const float K[4], float baseline, int mode_right, const sdso_trace_points_t* P) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, K && P && P->n >= 0, "null argument");
  PyramidDev* pyr = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &pyr));
  const int n = P->n;
  StereoState& S = stereo_state(ctx);
  if (!S.trace) S.trace = new TraceBatch();
  TraceBatch& B = *S.trace;
  SDSO_TRY(trace_reserve(ctx, B, std::max(n, 1)));
  trace_bind(B, n);
  SDSO_TRY(trace_set_camera(ctx, B.T, *pyr, K, baseline, mode_right));
  if (n) {
    for (const TbMember& m : kTbMembers)
      SDSO_HIP(ctx, hipMemcpyAsync(B.col(m.off), P->*m.host, sizeof(float) * (size_t)m.width * n, hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipMemcpyAsync(B.T.lastTraceStatus, P->lastTraceStatus, n, hipMemcpyHostToDevice, ctx->stream));
  }
  // pristine copies of the in/out fields
  SDSO_HIP(ctx, hipMemcpyAsync(B.pristine(), B.inout(), sizeof(float) * kTbInOutWidth * (size_t)B.n, hipMemcpyDeviceToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(B.pristine_status(), B.bytes, (size_t)B.n, hipMemcpyDeviceToDevice, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}
// the traceStereo kernel in the ctx's refinement mode (0 DSO-native GN, 1 the fork's g2o passes); at profiling level 1 the kernel's own
// duration goes under the name k_trace_stereo (the benchmarked enqueue, and a chain's two traces)
static void launch_trace_stereo(sdso_ctx* ctx, const TraceDev& T) {
  constexpr int P = 16;
  const dim3 g((T.n + P - 1) / P), b(256);
  if (ctx->gn_mode == 1) launch_timed(ctx, "k_trace_stereo", 1, (k_trace_stereo_blk<1, P>), g, b, T);
  else launch_timed(ctx, "k_trace_stereo", 1, (k_trace_stereo_blk<0, P>), g, b, T);
}
extern "C" int sdso_trace_stereo_enqueue(sdso_ctx* ctx) {
  if (!prepared_trace(ctx)) return sdso::fail(ctx, SDSO_ERR_STATE, "no prepared trace batch");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  TraceBatch& B = *prepared_trace(ctx);
  if (B.T.n == 0) return SDSO_OK;
  SDSO_HIP(ctx, hipMemcpyAsync(B.inout(), B.pristine(), sizeof(float) * kTbInOutWidth * (size_t)B.n, hipMemcpyDeviceToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(B.bytes, B.pristine_status(), (size_t)B.n, hipMemcpyDeviceToDevice, ctx->stream));
  launch_trace_stereo(ctx, B.T);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}
extern "C" int sdso_trace_stereo_fetch(sdso_ctx* ctx, sdso_trace_points_t* P, uint8_t* status) {
  if (!prepared_trace(ctx)) return sdso::fail(ctx, SDSO_ERR_STATE, "no prepared trace batch");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  TraceBatch& B = *prepared_trace(ctx);
  const int n = B.T.n;
  if (n && P) {
    for (const TbMember& m : kTbMembers)
      if (m.fetched && P->*m.host)
        SDSO_HIP(ctx, hipMemcpyAsync(P->*m.host, B.col(m.off), sizeof(float) * (size_t)m.width * n, hipMemcpyDeviceToHost, ctx->stream));
    if (P->lastTraceStatus) SDSO_HIP(ctx, hipMemcpyAsync(P->lastTraceStatus, B.T.lastTraceStatus, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (n && status) SDSO_HIP(ctx, hipMemcpyAsync(status, B.T.status, n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

extern "C" int sdso_trace_on_batch(sdso_ctx* ctx, int frame_slot, int ngeom, const sdso_trace_geom_t* geom, const int* point_geom,
                                   sdso_trace_points_t* pts, uint8_t* status) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, pts && pts->n >= 0 && ngeom >= 0, "null argument");
  const int n = pts->n;
  if (n == 0) return SDSO_OK;
  SDSO_REQUIRE(ctx, geom && point_geom && ngeom > 0, "null geometry");
  for (int i = 0; i < n; i++) SDSO_REQUIRE(ctx, point_geom[i] >= 0 && point_geom[i] < ngeom, "point_geom out of range");
  const float K0[4] = {1, 1, 0, 0};
  if (!pts->idepth_min) pts->idepth_min = pts->idepth_min_stereo;       // not used by traceOn; the upload needs a valid pointer
  if (!pts->idepth_stereo) pts->idepth_stereo = pts->idepth_min_stereo;
  int rc = sdso_trace_stereo_prepare(ctx, frame_slot, K0, 0.f, 1, pts);   // uploads the point state into the ctx's trace batch
  if (rc) return rc;
  TraceBatch& B = *prepared_trace(ctx);
  SDSO_TRY(ensure_scratch(ctx, sizeof(sdso_trace_geom_t) * (size_t)ngeom + sizeof(int) * (size_t)n));
  sdso_trace_geom_t* d_geom = (sdso_trace_geom_t*)ctx->scratch;
  int* d_pg = (int*)(d_geom + ngeom);
  SDSO_HIP(ctx, hipMemcpyAsync(d_geom, geom, sizeof(sdso_trace_geom_t) * ngeom, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemcpyAsync(d_pg, point_geom, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "k_trace_on");
    hipLaunchKernelGGL(k_trace_on, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, B.T, (const sdso_trace_geom_t*)d_geom, (const int*)d_pg);
  }
  SDSO_HIP(ctx, hipGetLastError());
  sdso_trace_points_t out = *pts;
  out.idepth_stereo = nullptr;
  return sdso_trace_stereo_fetch(ctx, &out, status);
}

// 0: DSO-native sub-pixel refinement (ImmaturePoint.cpp:707-769); 1: the fork's live g2o Gauss-Newton on
// EdgeTracePointUVDSO (ImmaturePoint.cpp:309-412).  Applies to every later traceStereo launch of this ctx.
extern "C" int sdso_trace_set_gn_mode(sdso_ctx* ctx, int mode) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, mode == 0 || mode == 1, "gn mode must be 0 (DSO-native) or 1 (g2o fork)");
  ctx->gn_mode = mode;
  return SDSO_OK;
}

extern "C" int sdso_trace_stereo_batch(sdso_ctx* ctx, int frame_slot, const float K[4], float baseline, int mode_right, sdso_trace_points_t* pts, uint8_t* status) {
  SDSO_TRY(sdso_trace_stereo_prepare(ctx, frame_slot, K, baseline, mode_right, pts));
  SDSO_TRY(sdso_trace_stereo_enqueue(ctx));
  return sdso_trace_stereo_fetch(ctx, pts, status);
}
