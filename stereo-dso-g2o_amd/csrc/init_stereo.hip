// sdso_init_*: the start of a sequence on the device.  The live part of CoarseInitializer::setFirstStereo (CoarseInitializer.cpp:838-972:
// level 0) and STEP 3 of FullSystem::initializeFromInitializer (FullSystem.cpp:1533-1573), on one state per ctx with buffers of its own.
//
// Not built, because nothing live reads it: levels >= 1 (makePixelStatus and the idepth[lvl] sums, CoarseInitializer.cpp:975-1013), makeNN
// (:1249), dGrads, setFirst, trackFrame and calcResAndGS.  Their only reader is the monocular trackFrame, which this fork never calls; the
// callers outside the class (FullSystem.cpp:1092-1093, :1498-1576) touch points[0] / numPoints[0] only.
//
// setFirstStereo: the map's entries inside [3, w-4) x [3, h-4) in raster order (the loop bounds of makeNewTraces: ImmMapPred states them
// once for both) become fresh points of the state's own TraceBatch (fresh_point, k_immature_init) and take one traceStereo into the right
// image (k_immature_init and k_trace_stereo_blk of stereo_trace.hip as they are: what launch_fresh_trace is made of).  Unlike
// sdso_imm_add_frame no point is dropped for its energyTH.  A point whose constructor met a non-finite pixel (energyTH NaN, a NaN among its
// colours) is a Pnt all the same, but takes no search: every step energy of such a point is NaN, no step becomes the best one, and the
// refinement then samples around (0, 0) — pixels (-2, -2) ff., in front of the image.  The reference reads there unchecked.  Its result
// does not depend on what it reads: `!(bestEnergy < energyTH * slack)` holds for a NaN energyTH whatever bestEnergy is, so the status is
// IPS_OOB where the search line fails its tests (trace_line) and IPS_OUTLIER otherwise, and the interval stays 0 / NaN.  k_init_skip marks
// those points for the trace kernel's skip bytes and init_status_unsearched states that verdict.
// k_init_pnts writes the Pnt records.  The batch stays as the trace left it: STEP 3 builds the same ImmaturePoint at the same pixel with
// the same interval and traces it into the same image, and traceStereo is deterministic, so colour, weights, energyTH, the interval,
// idepth_stereo and the status of the first trace ARE those of the second, which is not run.
namespace sdso {
enum { INIT_C_MAP = 0, INIT_C_PNTS = 1, INIT_C_HIST = 2 };                      // sdso_init_set_first_stereo's counts
enum { INIT_S_WALKED = 0, INIT_S_SKIPPED, INIT_S_DROPPED, INIT_S_MADE, kInitSelCounts };   // sdso_init_from_initializer's counts
static_assert(INIT_C_HIST + 6 == SDSO_INIT_NCOUNTS, "map entries, Pnts and one count per ImmaturePointStatus");
// the Pnts of n points in one run of bytes, so that sdso_init_get_pnts is one copy: u | v | idepth | iR | my_type (n floats each) | status
struct InitPnts { float *u, *v, *idepth, *iR, *my_type; uint8_t* status; };
constexpr size_t kInitPntBytes = 5 * sizeof(float) + 1;
static InitPnts init_pnts_view(char* p, int n) {
  float* f = (float*)p;
  const size_t N = (size_t)n;
  return InitPnts{f, f + N, f + 2 * N, f + 3 * N, f + 4 * N, (uint8_t*)(f + 5 * N)};
}
// a PointHessian of STEP 3 as 24 words, point-major, so that sdso_init_get_points copies the points made and no more:
// pnt (int) u v my_type idepth idepth_min idepth_max energyTH color[8] weights[8]
enum { INIT_R_PNT = 0, INIT_R_U, INIT_R_V, INIT_R_TYPE, INIT_R_IDEPTH, INIT_R_IMIN, INIT_R_IMAX, INIT_R_ETH, INIT_R_COLOR, INIT_R_WEIGHTS = INIT_R_COLOR + 8,
       kInitRecWords = INIT_R_WEIGHTS + 8 };

struct InitState {
  TraceBatch tb;                    // the Pnts as ImmaturePoints, as their traceStereo left them
  int cap = 0;                      // Pnts the buffers below hold
  DevBuf<float> d_type;             // my_type per Pnt
  DevBuf<char> d_pnt;               // InitPnts
  DevBuf<float> d_rec;              // kInitRecWords per point made
  DevBuf<uint8_t> d_keep, d_sel;    // the caller's flags; 1 = the Pnt becomes a point
  DevBuf<int> d_seg;                // segment counts / offsets of the compaction of STEP 3
  DevBuf<int> d_counts;             // SDSO_INIT_NCOUNTS | kInitSelCounts | candidates | points made
  PinBuf<int> h_counts;             // mirror of d_counts
  PinBuf<char> h_pnt;               // cap Pnts
  PinBuf<float> h_rec;              // cap records
  hipEvent_t ev = nullptr;          // behind the latest sdso_init_from_initializer's counts on their way to h_counts
  StageBuf stage;                   // a caller's map and flags on their way to the device
  bool valid = false, pts_valid = false, pts_pending = false;
  int n = 0, npts = 0, w = 0, h = 0;
};
constexpr int kInitCountInts = SDSO_INIT_NCOUNTS + kInitSelCounts + 2, kInitCandAt = SDSO_INIT_NCOUNTS + kInitSelCounts, kInitMadeAt = kInitCandAt + 1;

void release_init_stereo(sdso_ctx* ctx) {
  InitState* S = ctx->init;
  if (!S) return;
  if (S->ev) hipEventDestroy(S->ev);
  stage_free(S->stage);
  delete S;
  ctx->init = nullptr;
}
// the state's buffers for n Pnts; what an earlier call left in them is given up
static int init_reserve(sdso_ctx* ctx, InitState& S, int n) {
  SDSO_HIP(ctx, S.d_counts.reserve(ctx->stream, kInitCountInts, kInitCountInts));
  SDSO_HIP(ctx, S.h_counts.reserve(ctx->stream, kInitCountInts, kInitCountInts));
  if (!S.ev) SDSO_HIP(ctx, hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
  SDSO_TRY(trace_reserve(ctx, S.tb, n));
  if (S.cap >= n) return SDSO_OK;
  const size_t C = (size_t)n + n / 4 + 64, nseg = (C + 255) / 256 + 1;
  S.cap = 0;   // a group (devbuf.h)
  SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, S.d_type, S.d_pnt, S.d_rec, S.d_keep, S.d_sel, S.d_seg, S.h_pnt, S.h_rec));
  SDSO_HIP(ctx, S.d_type.reserve(ctx->stream, C, C));
  SDSO_HIP(ctx, S.d_pnt.reserve(ctx->stream, kInitPntBytes * C, kInitPntBytes * C));
  SDSO_HIP(ctx, S.d_rec.reserve(ctx->stream, kInitRecWords * C, kInitRecWords * C));
  SDSO_HIP(ctx, S.d_keep.reserve(ctx->stream, C, C));
  SDSO_HIP(ctx, S.d_sel.reserve(ctx->stream, C, C));
  SDSO_HIP(ctx, S.d_seg.reserve(ctx->stream, nseg, nseg));
  SDSO_HIP(ctx, S.h_pnt.reserve(ctx->stream, kInitPntBytes * C, kInitPntBytes * C));
  SDSO_HIP(ctx, S.h_rec.reserve(ctx->stream, kInitRecWords * C, kInitRecWords * C));
  S.cap = (int)C;
  return SDSO_OK;
}
static InitState* init_state_valid(sdso_ctx* ctx) { return ctx->init && ctx->init->valid ? ctx->init : nullptr; }

struct InitCandEmit {   // CoarseInitializer.cpp:897-902: ImmaturePoint(x, y, firstFrame, statusMap[i]) with the interval 0 / NaN
  const float* map; int w, cap; TraceDev T; float* type;
  __device__ void operator()(int idx, int pos) const {
    if (pos >= cap) return;
    fresh_point(T, pos, (float)(idx % w), (float)(idx / w), 0.f, 0.f, NAN);
    type[pos] = map[idx];
  }
};
struct InitSelPred {    // what k_init_select decided
  const uint8_t* sel;
  __device__ bool operator()(int idx) const { return sel[idx] != 0; }
};
struct InitPointEmit {  // PointHessian(pt) (HessianBlocks.cpp:35-68) and FullSystem.cpp:1565-1566 for Pnt idx, the pos-th point made
  TraceDev T; const float* type; float* rec; int cap;
  __device__ void operator()(int idx, int pos) const {
    if (pos >= cap) return;
    float* r = rec + (size_t)pos * kInitRecWords;
    r[INIT_R_PNT] = __int_as_float(idx);
    r[INIT_R_U] = T.u_stereo[idx]; r[INIT_R_V] = T.v_stereo[idx]; r[INIT_R_TYPE] = type[idx];
    r[INIT_R_IDEPTH] = T.idepth_stereo[idx]; r[INIT_R_IMIN] = T.idepth_min_stereo[idx]; r[INIT_R_IMAX] = T.idepth_max_stereo[idx];
    r[INIT_R_ETH] = T.energyTH[idx];
#pragma unroll
    for (int k = 0; k < 8; k++) { r[INIT_R_COLOR + k] = T.color[(size_t)idx * 8 + k]; r[INIT_R_WEIGHTS + k] = T.weights[(size_t)idx * 8 + k]; }
  }
};
}  // namespace sdso

// counts[0]: the non-zero entries of the whole map, the excluded border included (makeMaps' return value for its own map)
__global__ __launch_bounds__(256) void k_init_map_count(const float* __restrict__ map, int npx, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  imm_count(counts, INIT_C_MAP, i < npx && map[i] != 0);
}
// skip[j] = 1: the constructor left no finite energyTH; the point takes no search (the head of this file)
__global__ __launch_bounds__(256) void k_init_skip(int n, const float* __restrict__ energyTH, uint8_t* __restrict__ skip) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) skip[j] = isfinite(energyTH[j]) ? 0 : 1;
}
// what traceStereo returns for point j with a NaN energyTH: the status trace_line ends it with, else IPS_OUTLIER (ImmaturePoint.cpp:413-421;
// lastTraceStatus was IPS_UNINITIALIZED).  pr and Kt as k_trace_stereo_blk forms them (:98-117).
__device__ __forceinline__ int init_status_unsearched(const TraceDev& T, int j) {
  const float u_stereo = T.u_stereo[j], v_stereo = T.v_stereo[j];
  const float bl0 = T.mode_right ? -T.baseline : T.baseline;
  float Kt[3], pr[3];
  Kt[0] = (T.fx * bl0 + 0.0f * 0.0f) + T.cx * 0.0f;
  Kt[1] = (0.0f * bl0 + T.fy * 0.0f) + T.cy * 0.0f;
  Kt[2] = (0.0f * bl0 + 0.0f * 0.0f) + 1.0f * 0.0f;
  pr[0] = (1.0f * u_stereo + 0.0f * v_stereo) + 0.0f * 1.0f;
  pr[1] = (0.0f * u_stereo + 1.0f * v_stereo) + 0.0f * 1.0f;
  pr[2] = (0.0f * u_stereo + 0.0f * v_stereo) + 1.0f * 1.0f;
  TraceLine L;
  const int st = trace_line(pr, Kt, T.idepth_min[j], T.idepth_min_stereo[j], T.idepth_max_stereo[j], T.gradH + (size_t)j * 4, T.w, T.h, L);
  return st == kTraceSearch ? (int)IPS_OUTLIER : st;
}
// CoarseInitializer.cpp:905-969: the Pnt of every traced point — idepth = iR = idepth_stereo where the trace returned IPS_GOOD, 0.01f for
// every other status; u, v, my_type in both branches — and the histogram of the returned statuses
__global__ __launch_bounds__(256) void k_init_pnts(int n, TraceDev T, const float* __restrict__ type, InitPnts P, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < n;
  int st = -1;
  if (in) {
    st = T.status[j];
    if (st == 255) st = init_status_unsearched(T, j);   // skipped by k_init_skip
    const float d = st == IPS_GOOD ? T.idepth_stereo[j] : 0.01f;
    P.u[j] = T.u_stereo[j]; P.v[j] = T.v_stereo[j]; P.idepth[j] = d; P.iR[j] = d; P.my_type[j] = type[j];
    P.status[j] = (uint8_t)st;
  }
  imm_count(counts, INIT_C_PNTS, in);
#pragma unroll
  for (int k = 0; k < 6; k++) imm_count(counts, INIT_C_HIST + k, st == k);
}
// FullSystem.cpp:1535 and :1552-1559 for every Pnt: sel[j] = 1 where it passed the caller's rand() test (keep == nullptr: every Pnt did)
// and its ImmaturePoint has a finite energyTH and a finite interval with neither end negative
__global__ __launch_bounds__(256) void k_init_select(int n, TraceDev T, const uint8_t* __restrict__ keep, uint8_t* __restrict__ sel, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < n;
  bool kept = false, ok = false;
  if (in) {
    kept = !keep || keep[j] != 0;
    const float eth = T.energyTH[j], imin = T.idepth_min_stereo[j], imax = T.idepth_max_stereo[j];
    ok = !(!isfinite(eth) || !isfinite(imin) || !isfinite(imax) || imin < 0 || imax < 0);
    sel[j] = kept && ok ? 1 : 0;
  }
  imm_count(counts, INIT_S_WALKED, in);
  imm_count(counts, INIT_S_SKIPPED, in && !kept);
  imm_count(counts, INIT_S_DROPPED, kept && !ok);
  imm_count(counts, INIT_S_MADE, kept && ok);
}

// ------------------------------------------------------------------ API
extern "C" int sdso_init_set_first_stereo(sdso_ctx* ctx, int frame_slot, int right_slot, const float K[4], float baseline, const float* selection_map,
                                          int* numPoints, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  // ---- the refusals: nothing is launched, waited for or given up before them
  SDSO_REQUIRE(ctx, K, "null K");
  PyramidDev *PL = nullptr, *PR = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &PL));
  const int w = PL->w[0], h = PL->h[0];
  SDSO_TRY(frame_pyramid_sized(ctx, right_slot, w, h, "the right frame differs in size from the first frame", &PR, "unknown right frame slot"));
  SDSO_REQUIRE(ctx, w >= 16 && h >= 16, "image too small for the pattern");
  if (!selection_map) {
    SDSO_REQUIRE(ctx, PL->levels >= 3, "the selector reads absSquaredGrad of levels 0..2");
    if (w / 32 == 0 || h / 32 == 0) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_pixel_select state can be made on this frame slot: smaller than one 32x32 cell");
  }
  // ---- the map and the bound on its candidates
  const size_t npx = (size_t)w * h;
  const float* d_map = nullptr;
  int bound = 0;
  if (selection_map) {
    for (int y = 3; y < h - 4; y++)
      for (int x = 3; x < w - 4; x++) bound += selection_map[x + (size_t)y * w] != 0;
  } else {
    // CoarseInitializer.cpp:848, :865, :871: a fresh PixelSelector, currentPotential = 3, makeMaps(firstFrame, statusMap, densities[0]*w*h, 1, false, 2)
    int potential = 3, num = 0;
    SDSO_TRY(sdso_pixel_select(ctx, frame_slot, 0.03f * w * h, 1, 2.0f, &potential, nullptr, &num));
    if (!selector_final_map(ctx, frame_slot, w, h, &d_map, &bound)) return sdso::fail(ctx, SDSO_ERR_STATE, "sdso_pixel_select kept no map of this frame slot");
  }
  if (!ctx->init) ctx->init = new InitState();
  InitState& S = *ctx->init;
  S.valid = S.pts_valid = S.pts_pending = false;   // from here on the call replaces the state
  SDSO_TRY(init_reserve(ctx, S, std::max(bound, 1)));
  // scratch: [the caller's map] | row offsets
  SDSO_TRY(ensure_scratch(ctx, (selection_map ? sizeof(float) * npx : 0) + sizeof(int) * ((size_t)h + 4)));
  float* q = (float*)ctx->scratch;
  if (selection_map) {
    char* stage = nullptr;
    SDSO_TRY(stage_reserve(ctx, S.stage, sizeof(float) * npx, &stage));
    std::copy(selection_map, selection_map + npx, (float*)stage);
    SDSO_HIP(ctx, hipMemcpyAsync(q, stage, sizeof(float) * npx, hipMemcpyHostToDevice, ctx->stream));
    SDSO_TRY(stage_commit(ctx, S.stage));
    d_map = q; q += npx;
  }
  int* d_row = (int*)q;
  int* d_ncand = S.d_counts + kInitCandAt;
  SDSO_HIP(ctx, hipMemsetAsync(S.d_counts, 0, sizeof(int) * kInitCountInts, ctx->stream));
  launch_timed(ctx, "k_init_map_count", 2, k_init_map_count, dim3((unsigned)((npx + 255) / 256)), dim3(256), d_map, (int)npx, S.d_counts);
  int n = 0;
  if (bound > 0) {
    trace_bind(S.tb, bound);
    // a point whose constructor stops at a non-finite pixel leaves the rest of its colours and weights unwritten (ImmaturePoint.cpp:44-50)
    SDSO_HIP(ctx, hipMemsetAsync(S.tb.col(TB_COLOR), 0, sizeof(float) * 16 * (size_t)S.tb.n, ctx->stream));
    const ImmMapPred mp{d_map, w, h};
    const InitCandEmit me{d_map, w, bound, S.tb.T, S.d_type};
    launch_timed(ctx, "k_init_cand_count", 2, k_imm_segcount<ImmMapPred>, dim3(h), dim3(256), mp, (int)npx, w, d_row);
    launch_timed(ctx, "k_imm_scan", 2, k_imm_scan, dim3(1), dim3(256), d_row, h, d_ncand);
    launch_timed(ctx, "k_init_cand_write", 2, (k_imm_segwrite<ImmMapPred, InitCandEmit>), dim3(h), dim3(256), mp, me, (int)npx, w, (const int*)d_row);
    SDSO_HIP(ctx, hipGetLastError());
    n = bound;
    if (!selection_map) {   // the selector's count includes the excluded border: the launches below are sized by the candidates themselves
      SDSO_HIP(ctx, hipMemcpyAsync(S.h_counts + kInitCandAt, d_ncand, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
      n = std::min(S.h_counts[kInitCandAt], bound);
    }
  }
  if (n > 0) {
    trace_bind(S.tb, n);
    SDSO_TRY(trace_set_camera(ctx, S.tb.T, *PR, K, baseline, 1));
    // :897-903: the constructor on the left pyramid, the search in the right one for every point with a finite energyTH
    TraceDev& T = S.tb.T;
    launch_timed(ctx, "k_immature_init", 2, k_immature_init, dim3((n + 255) / 256), dim3(256), (const float4*)PL->d[0], w, n, (const float*)T.u_stereo, (const float*)T.v_stereo,
                 (float*)T.color, (float*)T.weights, (float*)T.gradH, (float*)T.energyTH);
    launch_timed(ctx, "k_init_skip", 2, k_init_skip, dim3((n + 255) / 256), dim3(256), n, T.energyTH, S.tb.skip());
    T.skip = S.tb.skip();
    launch_trace_stereo(ctx, T);
    launch_timed(ctx, "k_init_pnts", 2, k_init_pnts, dim3((n + 255) / 256), dim3(256), n, S.tb.T, (const float*)S.d_type, init_pnts_view(S.d_pnt, n), S.d_counts);
    SDSO_HIP(ctx, hipGetLastError());
  }
  S.n = n; S.w = w; S.h = h;
  S.valid = true;
  if (numPoints) *numPoints = n;
  if (counts) {
    SDSO_HIP(ctx, hipMemcpyAsync(S.h_counts, S.d_counts, sizeof(int) * SDSO_INIT_NCOUNTS, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(S.h_counts.get(), S.h_counts + SDSO_INIT_NCOUNTS, counts);
  }
  return SDSO_OK;
}

extern "C" int sdso_init_get_pnts(sdso_ctx* ctx, sdso_init_pnts_t* out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, out, "null argument");
  InitState* Sp = init_state_valid(ctx);
  if (!Sp) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_init_set_first_stereo on this ctx");
  InitState& S = *Sp;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const int n = out->n = S.n;
  if (n == 0) return SDSO_OK;
  SDSO_HIP(ctx, hipMemcpyAsync(S.h_pnt, S.d_pnt, kInitPntBytes * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const InitPnts P = init_pnts_view(S.h_pnt, n);
  const struct { float* dst; const float* src; } members[] = {{out->u, P.u}, {out->v, P.v}, {out->idepth, P.idepth}, {out->iR, P.iR}, {out->my_type, P.my_type}};
  for (const auto& m : members)
    if (m.dst) std::copy(m.src, m.src + n, m.dst);
  if (out->status) std::copy(P.status, P.status + n, out->status);
  return SDSO_OK;
}

namespace sdso {
// the counts of the latest sdso_init_from_initializer on the host side: waits for that call only
static int init_resolve_points(sdso_ctx* ctx, InitState& S) {
  if (!S.pts_pending) return SDSO_OK;
  SDSO_HIP(ctx, hipEventSynchronize(S.ev));
  S.npts = std::min(S.h_counts[kInitMadeAt], S.n);
  S.pts_pending = false;
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_init_from_initializer(sdso_ctx* ctx, const uint8_t* keep, int* n_points, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  InitState* Sp = init_state_valid(ctx);
  if (!Sp) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_init_set_first_stereo on this ctx");
  InitState& S = *Sp;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const int n = S.n;
  S.pts_valid = false;
  int* d_sel_counts = S.d_counts + SDSO_INIT_NCOUNTS;
  int* h_sel_counts = S.h_counts + SDSO_INIT_NCOUNTS;
  if (n == 0) {   // an empty loop in the reference
    S.pts_pending = false; S.npts = 0;
    std::fill(h_sel_counts, h_sel_counts + kInitSelCounts, 0);
  } else {
    const uint8_t* d_keep = nullptr;
    if (keep) {
      char* stage = nullptr;
      SDSO_TRY(stage_reserve(ctx, S.stage, (size_t)n, &stage));
      std::copy(keep, keep + n, (uint8_t*)stage);
      SDSO_HIP(ctx, hipMemcpyAsync(S.d_keep, stage, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
      SDSO_TRY(stage_commit(ctx, S.stage));
      d_keep = S.d_keep;
    }
    const int nseg = (n + 255) / 256;
    const dim3 g(nseg), b(256);
    SDSO_HIP(ctx, hipMemsetAsync(d_sel_counts, 0, sizeof(int) * kInitSelCounts, ctx->stream));
    launch_timed(ctx, "k_init_select", 2, k_init_select, g, b, n, S.tb.T, d_keep, S.d_sel, d_sel_counts);
    const InitSelPred sp{S.d_sel};
    const InitPointEmit se{S.tb.T, S.d_type, S.d_rec, n};
    launch_timed(ctx, "k_init_point_count", 2, k_imm_segcount<InitSelPred>, g, b, sp, n, 256, S.d_seg);
    launch_timed(ctx, "k_imm_scan", 2, k_imm_scan, dim3(1), b, S.d_seg, nseg, S.d_counts + kInitMadeAt);
    launch_timed(ctx, "k_init_point_write", 2, (k_imm_segwrite<InitSelPred, InitPointEmit>), g, b, sp, se, n, 256, (const int*)S.d_seg);
    SDSO_HIP(ctx, hipGetLastError());
    SDSO_HIP(ctx, hipMemcpyAsync(h_sel_counts, d_sel_counts, sizeof(int) * (kInitSelCounts + 2), hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipEventRecord(S.ev, ctx->stream));
    S.pts_pending = true;
  }
  S.pts_valid = true;
  if (!n_points && !counts) return SDSO_OK;
  SDSO_TRY(init_resolve_points(ctx, S));
  if (n_points) *n_points = S.npts;
  if (counts) std::copy(h_sel_counts, h_sel_counts + kInitSelCounts, counts);
  return SDSO_OK;
}

extern "C" int sdso_init_get_points(sdso_ctx* ctx, sdso_init_points_t* out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, out, "null argument");
  InitState* Sp = init_state_valid(ctx);
  if (!Sp) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_init_set_first_stereo on this ctx");
  InitState& S = *Sp;
  if (!S.pts_valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_init_from_initializer on this state");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_TRY(init_resolve_points(ctx, S));
  const int n = out->n = S.npts;
  if (n == 0) return SDSO_OK;
  SDSO_HIP(ctx, hipMemcpyAsync(S.h_rec, S.d_rec, sizeof(float) * kInitRecWords * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const struct { float* dst; int at, width; } members[] = {{out->u, INIT_R_U, 1},       {out->v, INIT_R_V, 1},       {out->my_type, INIT_R_TYPE, 1}, {out->idepth, INIT_R_IDEPTH, 1},
                                                           {out->idepth_min, INIT_R_IMIN, 1}, {out->idepth_max, INIT_R_IMAX, 1}, {out->energyTH, INIT_R_ETH, 1},
                                                           {out->color, INIT_R_COLOR, 8}, {out->weights, INIT_R_WEIGHTS, 8}};
  for (int i = 0; i < n; i++) {
    const float* r = S.h_rec + (size_t)i * kInitRecWords;
    if (out->pnt) std::memcpy(&out->pnt[i], &r[INIT_R_PNT], sizeof(int));
    for (const auto& m : members)
      if (m.dst) std::copy(r + m.at, r + m.at + m.width, m.dst + (size_t)i * m.width);
  }
  return SDSO_OK;
}

extern "C" int sdso_init_release(sdso_ctx* ctx) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->init) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // launches that read the state's buffers may still be in flight
  release_init_stereo(ctx);
  return SDSO_OK;
}
