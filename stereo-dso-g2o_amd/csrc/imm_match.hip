// sdso_imm_stereo_match: the loop of FullSystem::stereoMatch (FullSystem.cpp:581-613) on one group of the resident set.  The group's own
// points are traced into the right image and fresh points of the right image back into the left (trace_pair_bind / launch_trace_stereo /
// launch_fresh_trace on the set's two batches, as sdso_imm_trace); this file's prepare / back / accept kernels stand around the two traces.
// The group is read only.  The results go to buffers of their own (ImmMatchKept, imm_set.hip) and stay there until the next call.
namespace sdso {
enum { IMM_M_WALKED = 0, IMM_M_FWD_GOOD, IMM_M_BACK_RUN, IMM_M_BACK_GOOD, IMM_M_ACCEPTED, IMM_M_FAR, IMM_M_DEPTH, IMM_M_UNREADABLE };
static_assert(IMM_M_UNREADABLE + 1 == SDSO_IMM_MATCH_NCOUNTS, "one name per count of sdso_imm_stereo_match");
// the per-point results of n points in one run of bytes: counts | idepth n*3 | accepted n | status_fwd n | status_back n.  What stereoMatch
// itself reads (13 bytes per point) comes first, so that a caller who asks for no status copies that much and no more.
struct ImmMatchRes { int* counts; float* idepth; uint8_t *accepted, *status_fwd, *status_back; };
static size_t imm_match_bytes(int n, bool statuses) { return sizeof(int) * SDSO_IMM_MATCH_NCOUNTS + (size_t)n * (statuses ? 15 : 13); }
static ImmMatchRes imm_match_view(char* p, int n) {
  ImmMatchRes R;
  R.counts = (int*)p;
  R.idepth = (float*)(p + sizeof(int) * SDSO_IMM_MATCH_NCOUNTS);
  R.accepted = (uint8_t*)(R.idepth + 3 * (size_t)n);
  R.status_fwd = R.accepted + n;
  R.status_back = R.status_fwd + n;
  return R;
}
}  // namespace sdso

// :582-585: the forward points are the group's points themselves — stored colour, weights, gradH, energyTH, quality and last trace — with
// u_stereo / v_stereo = u / v and the interval 0 / NaN, whatever the set stores
__global__ __launch_bounds__(256) void k_imm_match_prepare(ImmHostDev H, TraceDev F, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < H.n;
  imm_count(counts, IMM_M_WALKED, in);
  if (!in) return;
  const float* __restrict__ f = H.f;
  const size_t N = (size_t)H.cap, p = (size_t)j;
  F.u_stereo[j] = f[IMM_U * N + p]; F.v_stereo[j] = f[IMM_V * N + p];
  F.idepth_min[j] = 0.f; F.idepth_min_stereo[j] = 0.f; F.idepth_max_stereo[j] = NAN; F.idepth_stereo[j] = 0.f;
  F.quality[j] = f[IMM_QUAL * N + p];
  float *color = (float*)F.color, *weights = (float*)F.weights, *gradH = (float*)F.gradH;   // the batch's own columns
#pragma unroll
  for (int k = 0; k < 8; k++) { color[p * 8 + k] = f[IMM_COLOR * N + p * 8 + k]; weights[p * 8 + k] = f[IMM_WEIGHTS * N + p * 8 + k]; }
#pragma unroll
  for (int k = 0; k < 4; k++) gradH[p * 4 + k] = f[IMM_GRADH * N + p * 4 + k];
  ((float*)F.energyTH)[j] = f[IMM_ETH * N + p];
  F.lastTraceStatus[j] = H.st[j];
  F.lastTraceUV[2 * j] = f[IMM_UV * N + p * 2]; F.lastTraceUV[2 * j + 1] = f[IMM_UV * N + p * 2 + 1];
  F.lastTracePixelInterval[j] = f[IMM_INTERVAL * N + p];
}
// :589-595: the back points, fresh ones with the interval 0 / NaN
__global__ __launch_bounds__(256) void k_imm_match_back(int n, int w, int h, TraceDev F, TraceDev Bk, uint8_t* __restrict__ skipB, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool good = false, run = false;
  if (j < n) imm_back_point(j, w, h, F, Bk, nullptr, skipB, nullptr, nullptr, good, run);
  imm_count(counts, IMM_M_FWD_GOOD, good);
  imm_count(counts, IMM_M_BACK_RUN, run);
  imm_count(counts, IMM_M_UNREADABLE, good && !run);
}
// :598-611: the accept rule, the per-point results and, with a map, the accepted point's three floats at pixel ((int)v, (int)u).  A point
// whose pixel is not in the image (a group of sdso_imm_put_host may hold one) writes no pixel.
__global__ __launch_bounds__(256) void k_imm_match_accept(int n, int w, int h, TraceDev F, TraceDev Bk, float max_depth, ImmMatchRes R, float* __restrict__ map) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool back_good = false, near = false, in_range = false;
  if (j < n) {
    const uint8_t sf = F.status[j], sb = Bk.status[j];   // the back trace writes 255 for a point it skipped
    back_good = sb == IPS_GOOD;
    const float u = F.u_stereo[j], v = F.v_stereo[j];
    float out[3] = {0.f, 0.f, 0.f};
    if (back_good) {
      const float u_stereo_delta = fabsf(u - Bk.lastTraceUV[2 * j]);
      const float depth = 1.0f / F.idepth_stereo[j];
      near = u_stereo_delta < 1;
      in_range = depth > 0 && depth < max_depth;
      if (near && in_range) { out[0] = F.idepth_stereo[j]; out[1] = F.idepth_min_stereo[j]; out[2] = F.idepth_max_stereo[j]; }
    }
    const bool acc = back_good && near && in_range;
    R.accepted[j] = acc ? 1 : 0;
    R.status_fwd[j] = sf; R.status_back[j] = sb;
#pragma unroll
    for (int k = 0; k < 3; k++) R.idepth[3 * (size_t)j + k] = out[k];
    if (acc && map && u >= 0 && u < w && v >= 0 && v < h) {
      float* px = map + ((size_t)(int)v * w + (int)u) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = out[k];
    }
  }
  imm_count(R.counts, IMM_M_BACK_GOOD, back_good);
  imm_count(R.counts, IMM_M_ACCEPTED, back_good && near && in_range);
  imm_count(R.counts, IMM_M_FAR, back_good && !near);
  imm_count(R.counts, IMM_M_DEPTH, back_good && near && !in_range);
}

namespace sdso {
// both result buffers for n points; the kept results are given up first (a call that comes this far replaces them)
static int imm_match_reserve(sdso_ctx* ctx, ImmMatchKept& M, int n) {
  M.valid = false; M.have = 0;
  if (M.d && M.cap >= n) return SDSO_OK;
  const int cap = n + n / 4 + 64;
  M.cap = 0;   // a group (devbuf.h)
  SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, M.d, M.h));
  SDSO_HIP(ctx, M.d.reserve(ctx->stream, imm_match_bytes(cap, true), imm_match_bytes(cap, true)));
  SDSO_HIP(ctx, M.h.reserve(ctx->stream, imm_match_bytes(cap, true), imm_match_bytes(cap, true)));
  M.cap = cap;
  return SDSO_OK;
}
static int imm_match_map_reserve(sdso_ctx* ctx, ImmMatchKept& M, int w, int h) {
  M.map_valid = false;
  const size_t floats = (size_t)w * h * 3;
  SDSO_HIP(ctx, M.d_map.reserve(ctx->stream, floats, floats));
  M.map_w = w; M.map_h = h;
  return SDSO_OK;
}
// the kept results into the caller's arrays: at most one copy of the per-point results (none where the mirror already holds them), a second
// one for the dense map, one synchronisation
static int imm_match_copy_out(sdso_ctx* ctx, ImmMatchKept& M, sdso_imm_match_out_t* out, int* counts) {
  const int n = M.n;
  const size_t need = imm_match_bytes(n, out && (out->status_fwd || out->status_back));
  const bool fetch = need > M.have, map = out && out->map;
  if (fetch) SDSO_HIP(ctx, hipMemcpyAsync(M.h, M.d, need, hipMemcpyDeviceToHost, ctx->stream));
  if (map) SDSO_HIP(ctx, hipMemcpyAsync(out->map, M.d_map, sizeof(float) * 3 * (size_t)M.map_w * M.map_h, hipMemcpyDeviceToHost, ctx->stream));
  if (fetch || map) SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (fetch) M.have = need;
  const ImmMatchRes R = imm_match_view(M.h, n);
  if (counts) std::copy(R.counts, R.counts + SDSO_IMM_MATCH_NCOUNTS, counts);
  if (out) {
    if (out->accepted) std::copy(R.accepted, R.accepted + n, out->accepted);
    if (out->idepth) std::copy(R.idepth, R.idepth + 3 * (size_t)n, out->idepth);
    if (out->status_fwd) std::copy(R.status_fwd, R.status_fwd + n, out->status_fwd);
    if (out->status_back) std::copy(R.status_back, R.status_back + n, out->status_back);
  }
  return SDSO_OK;
}
}  // namespace sdso

extern "C" int sdso_imm_stereo_match(sdso_ctx* ctx, int host_id, int frame_slot, int right_slot, const float K[4], float baseline, float max_depth, int build_map,
                                     sdso_imm_match_out_t* out, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  // ---- the refusals: nothing is launched, waited for or given up before them
  SDSO_REQUIRE(ctx, K, "null K");
  SDSO_REQUIRE(ctx, max_depth > 0, "max_depth must be > 0");
  SDSO_REQUIRE(ctx, build_map || !(out && out->map), "out->map needs build_map");
  ImmHost* Hp = nullptr;
  if (ctx->imm) { auto it = ctx->imm->hosts.find(host_id); if (it != ctx->imm->hosts.end()) Hp = &it->second; }
  SDSO_REQUIRE(ctx, Hp, "unknown host_id");
  ImmHost& H = *Hp;
  const int w = H.w, h = H.h;
  PyramidDev *PL = nullptr, *PR = nullptr;
  SDSO_TRY(frame_pyramid_sized(ctx, frame_slot, w, h, "the frame differs in size from the host's", &PL));
  SDSO_TRY(frame_pyramid_sized(ctx, right_slot, w, h, "the right frame differs in size from the host's", &PR, "unknown right frame slot"));
  // ---- the call
  ImmState& S = *ctx->imm;
  ImmMatchKept& M = S.match;
  SDSO_TRY(imm_resolve(ctx, H));
  const int n = H.n;
  SDSO_TRY(imm_match_reserve(ctx, M, n));
  if (build_map) SDSO_TRY(imm_match_map_reserve(ctx, M, w, h));
  const ImmMatchRes R = imm_match_view(M.d, n);
  SDSO_HIP(ctx, hipMemsetAsync(M.d, 0, imm_match_bytes(n, true), ctx->stream));
  float* map = build_map ? M.d_map : nullptr;
  if (map) SDSO_HIP(ctx, hipMemsetAsync(map, 0, sizeof(float) * 3 * (size_t)w * h, ctx->stream));
  if (n) {
    SDSO_TRY(trace_pair_bind(ctx, S.fwd, S.back, n, *PL, *PR, K, baseline, 1, 0));
    const TraceDev& F = S.fwd.T;     // forward: the group's points searched in the right frame
    const TraceDev& Bk = S.back.T;   // back: points of the right frame searched in the left one
    uint8_t* skipB = S.back.skip();
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_match_prepare", 2, k_imm_match_prepare, g1, b1, ImmHostDev{H.f[0], H.st[0], n, H.cap}, F, R.counts);
    launch_trace_stereo(ctx, F);
    launch_timed(ctx, "k_imm_match_back", 2, k_imm_match_back, g1, b1, n, w, h, F, Bk, skipB, R.counts);
    launch_fresh_trace(ctx, Bk, *PR, skipB);
    launch_timed(ctx, "k_imm_match_accept", 2, k_imm_match_accept, g1, b1, n, w, h, F, Bk, max_depth, R, map);
    SDSO_HIP(ctx, hipGetLastError());
  }
  M.valid = true; M.n = n;
  M.map_latest = build_map != 0;
  if (build_map) M.map_valid = true;
  if (!out && !counts) return SDSO_OK;
  return imm_match_copy_out(ctx, M, out, counts);
}

extern "C" int sdso_imm_stereo_match_fetch(sdso_ctx* ctx, sdso_imm_match_out_t* out, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->imm || !ctx->imm->match.valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_imm_stereo_match results to fetch");
  ImmMatchKept& M = ctx->imm->match;
  SDSO_REQUIRE(ctx, !(out && out->map) || M.map_latest, "out->map: the latest sdso_imm_stereo_match built no map");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  return imm_match_copy_out(ctx, M, out, counts);
}

extern "C" int sdso_imm_stereo_map_dev(sdso_ctx* ctx, void** map_dev, int* w, int* h) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, map_dev && w && h, "null argument");
  if (!ctx->imm || !ctx->imm->match.map_valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_imm_stereo_match has built a map");
  const ImmMatchKept& M = ctx->imm->match;
  *map_dev = M.d_map; *w = M.map_w; *h = M.map_h;
  return SDSO_OK;
}
