// BA host API, part 8 (included by ba.hip): sdso_ba_flag_points — FullSystem::removeOutliers and FullSystem::flagPointsForRemoval decided
// on the device-resident window (gfx950).  The rule itself is ba_flag.h; this file walks the window to its inputs and counts the outcome.
//
// Every input is in the window when an optimize call has ended (ba_kernels.h): the point's residuals in residualsAll order through
// p_rbeg / p_rcnt / p_rlist with their targets in the nibbles of p_order (as k_ref_gather finds lastResiduals[0]), r_state / r_act /
// r_lin (toRemove = in activeResiduals and not active, FullSystemOptimize.cpp:80-84), p_track (numGoodResiduals, idepth_hessian), p_geo.z.
//
//   k_ba_flag_points  one lane per point, 256 per workgroup; latency-bound (<= 8 dependent byte loads per lane, a window holds <= ~16 k
//                     points).  The flagged frames travel as a bit mask and the settings as arguments: the only upload is last_gone.
//                     Counting: one wave ballot + popc per (host, code) into a per-workgroup LDS histogram, then integer atomics
//                     into the window's buffer — no float, so the result is the same bytes on every run.
// The window owns ONE buffer for the call: [counts 6 | host_counts 8 x 6 | pad to 256 B | decision np | last_gone 2 np].  The head up to
// the decisions is cleared on the stream before the launch and comes back in one copy.
#include "ba_flag.h"

namespace sdso {

constexpr int FLAG_BLOCK = 256;
constexpr int FLAG_NCODE = 6;
constexpr int FLAG_HEAD_INTS = FLAG_NCODE + 8 * FLAG_NCODE;   // counts, then host_counts for the 8 frames a window can hold
constexpr size_t FLAG_HEAD_BYTES = 256;
static_assert(FLAG_HEAD_INTS * sizeof(int) <= FLAG_HEAD_BYTES, "the counters fit the head of the buffer");

__global__ __launch_bounds__(FLAG_BLOCK) void k_ba_flag_points(const BaDev* __restrict__ win, unsigned frame_marg_mask, FlagSettings S,
                                                               const uint8_t* __restrict__ last_gone, int* __restrict__ head, uint8_t* __restrict__ decision) {
  const BaDev& B = *win;
  __shared__ int s_hc[8 * FLAG_NCODE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nf = B.nf, np = B.np;
  if (tid < 8 * FLAG_NCODE) s_hc[tid] = 0;
  __syncthreads();
  const int p = blockIdx.x * FLAG_BLOCK + tid;
  const bool valid = p < np;
  int code = -1, host = -1;
  if (valid) {
    const unsigned ord = gld(B.p_order + p);
    const int rbeg = gld(B.p_rbeg + p), rcnt = gld(B.p_rcnt + p);
    host = gld(B.p_host + p);
    const f32x4 tr = gld((const f32x4*)B.p_track + p);
    const float idepth = gld((const float*)B.p_geo + (size_t)p * 4 + 2);
    FlagPointAcc a;
#pragma unroll
    for (int k = 0; k < SDSO_MAX_RES; k++) {
      if (k < rcnt) {
        const int j = gld(B.p_rlist + rbeg + k);                                 // pair-sorted index of the k-th residual of residualsAll
        const bool removed = !(gld(B.r_lin + j) & 1) && !gld(B.r_act + j);       // on toRemove (FullSystemOptimize.cpp:80-84)
        flag_point_add(a, (int)((ord >> (4 * k)) & 15u), (int)gld(B.r_state + j), removed, nf, frame_marg_mask);
      }
    }
    const int g0 = last_gone ? (int)gld(last_gone + (size_t)p * 2) : FLAG_NONE, g1 = last_gone ? (int)gld(last_gone + (size_t)p * 2 + 1) : FLAG_NONE;
    code = flag_point_decide(a.n, a.visInToMarg, flag_point_last(a.last[0], g0), flag_point_last(a.last[1], g1), idepth, __float_as_int(tr.y), tr.z,
                             (frame_marg_mask >> host) & 1u, S);
    gst(decision + p, (uint8_t)code);
  }
  // points are grouped by host: a wave sees few of them, and a (host, code) pair nobody holds costs one ballot
  for (int h = 0; h < nf; h++) {
    if (!__ballot(host == h)) continue;                                          // (wave-uniform)
#pragma unroll
    for (int c = 0; c < FLAG_NCODE; c++) {
      const unsigned long long m = __ballot(host == h && code == c);
      if (lane == 0 && m) atomicAdd(&s_hc[h * FLAG_NCODE + c], __popcll(m));
    }
  }
  __syncthreads();
  if (tid < 8 * FLAG_NCODE) {
    const int v = s_hc[tid];
    if (v) { atomicAdd(head + FLAG_NCODE + tid, v); atomicAdd(head + tid % FLAG_NCODE, v); }
  }
}

}  // namespace sdso

extern "C" int sdso_ba_flag_points(sdso_ctx* ctx, int win, const sdso_ba_flag_points_t* prm, uint8_t* decision, int* counts, int* host_counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  // ---- refusals: all before any device work
  BaRefView V;
  int rc = ba_ref_view(ctx, win, &V);
  if (rc) return rc;
  SDSO_REQUIRE(ctx, prm, "null sdso_ba_flag_points_t");
  SDSO_REQUIRE(ctx, prm->frame_marg, "null frame_marg");
  SDSO_REQUIRE(ctx, decision, "null decision");
  SDSO_REQUIRE(ctx, prm->minGoodActiveResForMarg >= 0 && prm->minGoodResForMarg >= 0 && prm->minIdepthH_marg >= 0, "negative setting");
  const int nf = V.nf, np = V.np;
  if (prm->last_gone)
    for (size_t i = 0; i < (size_t)np * 2; i++) SDSO_REQUIRE(ctx, prm->last_gone[i] <= 2 || prm->last_gone[i] == 255, "last_gone entry outside {0, 1, 2, 255}");
  unsigned mask = 0;
  for (int f = 0; f < nf; f++) mask |= prm->frame_marg[f] ? 1u << f : 0u;
  // ---- the window's buffer
  BaWindowDev* W = find_win(ctx, win);
  const size_t gone_off = FLAG_HEAD_BYTES + (((size_t)np + 255) & ~(size_t)255);
  if (!W->d_flag) { DM(W->d_flag, uint8_t, gone_off + (size_t)np * 2); }
  uint8_t* d_dec = W->d_flag + FLAG_HEAD_BYTES;
  uint8_t* d_gone = W->d_flag + gone_off;
  SDSO_HIP(ctx, hipMemsetAsync(W->d_flag, 0, FLAG_HEAD_BYTES + (size_t)np, ctx->stream));
  if (prm->last_gone && np) SDSO_HIP(ctx, hipMemcpyAsync(d_gone, prm->last_gone, (size_t)np * 2, hipMemcpyHostToDevice, ctx->stream));
  if (np) {
    const FlagSettings S{prm->minGoodActiveResForMarg, prm->minGoodResForMarg, prm->minIdepthH_marg};
    launch_timed(ctx, "k_ba_flag_points", 2, k_ba_flag_points, dim3((np + FLAG_BLOCK - 1) / FLAG_BLOCK), dim3(FLAG_BLOCK), V.dev, mask, S,
                 (const uint8_t*)(prm->last_gone ? d_gone : nullptr), (int*)W->d_flag, d_dec);
    SDSO_HIP(ctx, hipGetLastError());
  }
  // ---- the one read-back
  std::vector<uint8_t> back(FLAG_HEAD_BYTES + (size_t)np);
  SDSO_HIP(ctx, hipMemcpyAsync(back.data(), W->d_flag, back.size(), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (np) std::memcpy(decision, back.data() + FLAG_HEAD_BYTES, (size_t)np);
  if (counts) std::memcpy(counts, back.data(), sizeof(int) * FLAG_NCODE);
  if (host_counts) std::memcpy(host_counts, back.data() + sizeof(int) * FLAG_NCODE, sizeof(int) * (size_t)nf * FLAG_NCODE);
  return SDSO_OK;
}
