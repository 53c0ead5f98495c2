// CoarseTracker::setCoarseTrackingRef -> makeCoarseDepthL0 from the device-resident BA window (gfx950): STEP1's gather, the
// static-stereo re-observation and the accept rule stay on the device, then STEP2-5 (coarse_depth.hip).
//
// Reference: src/FullSystem/CoarseTracker.cpp
//   :288-300  for every frame, every pointHessian: lastResiduals[0].first != 0 && lastResiduals[0].second == ResState::IN
//   :303-312  u = int(centerProjectedTo[0] + 0.5f), v likewise; ImmaturePoint(u, v, fh_target); the interval [0.1, 1.9] * centerProjectedTo[2]
//   :313-327  traceStereo into fh_right; where GOOD, an ImmaturePoint at lastTraceUV on fh_right traced back into fh_target
//   :329-341  depth = 1.0f / idepth_stereo; u_delta = abs(u - back lastTraceUV(0)); u_delta < 1 && depth > 0 && depth < 50 takes idepth_stereo
//   :350      weight = sqrtf(1e-3 / (ph->efPoint->HdiF + 1e-12))
//
// Every input of that loop is in the window after FullSystem::optimize (ba_kernels.h): lastResiduals[0] is the point's residual into
// the newest keyframe (FullSystem.cpp:1370-1387 gives every point one; linearizeAll(true) clears .first of those it drops), found
// through the target nibbles of p_order and p_rlist; centerProjectedTo is the expression of k_ba_post_state (Residuals.cpp:130-131).
//
// Two small latency-bound kernels, one lane per point / record; between them runs the L->R->L chain of sdso_stereo_match_batch.
//   k_ref_gather  ONE workgroup of 1024 lanes walks the ordered points in strips of 1024 and carries the running count from strip to
//                 strip, so a selected point's record lands at its rank in the caller's order without atomics and without a second
//                 pass (a window holds <= ~16 k points: 16 strips; three launches of a multi-block count / scan / scatter cost more
//                 than the strips).  LDS: the 16 wave counts of the rank scan, twice.  Records are SoA: every store is coalesced.
//   k_ref_accept  the accept rule per record; copies the two statuses next to the records (the match batches are reused by the
//                 next chain of the ctx).
#include "ba_kernels.h"
#include <algorithm>
#include <map>
#include <vector>

using namespace sdso;

namespace sdso {

constexpr int RG_BLOCK = 1024;
enum { RW_POINT = 0, RW_U, RW_V, RW_ORDER, RW_NINT };                          // int arrays of a record set
enum { RW_FU = 0, RW_FV, RW_IMIN, RW_IMAX, RW_CPT2, RW_WGT, RW_NEWID, RW_NFLT };   // float arrays
enum { RW_SKIP = 0, RW_SFWD, RW_SBACK, RW_NBYTE };                             // byte arrays

// STEP1's records of one reference slot, in splat order; all arrays hold `cap` entries
struct RefRecDev {
  int* i32;       // RW_NINT x cap, then 4 counters: [0] selected points, [1] of them border points, [2] selected but outside the image
  float* f32;     // RW_NFLT x cap
  uint8_t* u8;    // RW_NBYTE x cap
  int cap;
  __host__ __device__ int* ints(int k) const { return i32 + (size_t)k * cap; }
  __host__ __device__ float* flts(int k) const { return f32 + (size_t)k * cap; }
  __host__ __device__ uint8_t* bytes(int k) const { return u8 + (size_t)k * cap; }
  __host__ __device__ int* counts() const { return i32 + (size_t)RW_NINT * cap; }
};
// stale: the slot has taken a template from elsewhere since (sdso_track_import_ref): the records are not that template's
struct RefRecSet {
  DevBuf<int> i32; DevBuf<float> f32; DevBuf<uint8_t> u8;   // what `d` views (reserve_records)
  RefRecDev d{nullptr, nullptr, nullptr, 0};
  int n = 0;
  bool stale = false;
};
struct RefWinState { std::map<int, RefRecSet> sets; };

void refwin_forget_slot(sdso_ctx* ctx, int ref_slot) {
  if (!ctx->refwin) return;
  auto it = ctx->refwin->sets.find(ref_slot);
  if (it != ctx->refwin->sets.end()) it->second.stale = true;   // (the buffers stay for the slot's next sdso_track_make_ref_from_window)
}

void release_refwin(sdso_ctx* ctx) {
  delete ctx->refwin;
  ctx->refwin = nullptr;
}

}  // namespace sdso

namespace {

// n_items ordered points (order == nullptr: the window's own order) -> the records of the selected ones, at their rank
__global__ __launch_bounds__(RG_BLOCK) void k_ref_gather(const BaDev* __restrict__ win, const int* __restrict__ order, int n_items, RefRecDev R) {
  const BaDev& B = *win;
  __shared__ int s_sel[RG_BLOCK / 64], s_brd[RG_BLOCK / 64], s_out[RG_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nf = B.nf, tgt = nf - 1, w = B.w, h = B.h;
  int carry = 0, nborder = 0, noutside = 0;
  for (int base = 0; base < n_items; base += RG_BLOCK) {
    const int i = base + tid;
    bool sel = false;
    int p = 0, j = 0;
    if (i < n_items) {
      p = order ? gld(order + i) : i;
      const unsigned ord = gld(B.p_order + p);
      int k = -1;
#pragma unroll
      for (int kk = 7; kk >= 0; kk--) if ((int)((ord >> (4 * kk)) & 15u) == tgt) k = kk;   // a point observes a target at most once
      if (k >= 0) {
        j = gld(B.p_rlist + gld(B.p_rbeg + p) + k);                     // pair-sorted index of that residual
        sel = !(gld(B.r_lin + j) & 1) && gld(B.r_act + j) && gld(B.r_state + j) == 0;   // in activeResiduals, active, ResState::IN
      }
    }
    float cu = 0.f, cv = 0.f, cid = 0.f, wgt = 0.f;
    int u = 0, v = 0;
    bool border = false, outside = false;
    if (sel) {
      const int hst = gld(B.r_host + j);
      const float* __restrict__ pre = B.t_precalc + (size_t)(hst * nf + tgt) * 27;
      const float* R0 = pre + 12; const float* t0 = pre + 21;
      const float4 g = B.p_geo[p];
      const float pu = g.x, pv = g.y, idepth_zero_scaled = g.w;
      // projectPoint at the FEJ point (ResidualProjections.h:64-96), as k_ba_post_state evaluates centerProjectedTo
      float KliP[3];
      KliP[0] = (pu + 0 - B.cxl) * B.fxli;
      KliP[1] = (pv + 0 - B.cyl) * B.fyli;
      KliP[2] = 1;
      float ptp[3];
#pragma unroll
      for (int r = 0; r < 3; r++) ptp[r] = ((gld(R0 + r * 3 + 0) * KliP[0] + gld(R0 + r * 3 + 1) * KliP[1]) + gld(R0 + r * 3 + 2) * KliP[2]) + gld(t0 + r) * idepth_zero_scaled;
      const float drescale = 1.0f / ptp[2];
      const float pxu = ptp[0] * drescale, pxv = ptp[1] * drescale;
      cu = pxu * B.fxl + B.cxl; cv = pxv * B.fyl + B.cyl; cid = idepth_zero_scaled * drescale;
      u = (int)(cu + 0.5f); v = (int)(cv + 0.5f);                         // CoarseTracker.cpp:303-304
      const float hdi = gld(B.p_out + (size_t)p * 16 + PO_HDI);
      wgt = sqrtf((float)(1e-3 / ((double)hdi + 1e-12)));                 // :350 (double division, sqrtf of the float)
      outside = !(u >= 0 && v >= 0 && u < w && v < h);                    // the reference would write outside its maps: not splatted
      border = !outside && !(u >= 2 && v >= 2 && u < w - 3 && v < h - 3);   // ... and read outside the image: no stereo
      if (outside) sel = false;
    }
    const unsigned long long m = __ballot(sel);
    const unsigned long long mb = __ballot(border), mo = __ballot(outside);
    if (lane == 0) { s_sel[wv] = __popcll(m); s_brd[wv] = __popcll(mb); s_out[wv] = __popcll(mo); }
    __syncthreads();
    int rank = carry + __popcll(m & ((1ull << lane) - 1ull)), strip = 0;
#pragma unroll
    for (int k = 0; k < RG_BLOCK / 64; k++) { rank += k < wv ? s_sel[k] : 0; strip += s_sel[k]; nborder += s_brd[k]; noutside += s_out[k]; }
    if (sel) {
      gst(R.ints(RW_POINT) + rank, p); gst(R.ints(RW_U) + rank, u); gst(R.ints(RW_V) + rank, v);
      // a border point is parked on a harmless pixel: the ImmaturePoint constructor of the chain reads its pattern before the skip
      gst(R.flts(RW_FU) + rank, border ? 8.f : (float)u); gst(R.flts(RW_FV) + rank, border ? 8.f : (float)v);
      gst(R.flts(RW_IMIN) + rank, cid * 0.1f); gst(R.flts(RW_IMAX) + rank, cid * 1.9f);   // :311-312
      gst(R.flts(RW_CPT2) + rank, cid); gst(R.flts(RW_WGT) + rank, wgt);
      gst(R.bytes(RW_SKIP) + rank, (uint8_t)(border ? 1 : 0));
    }
    carry += strip;
    __syncthreads();
  }
  if (tid == 0) { int* c = R.counts(); gst(c, carry); gst(c + 1, nborder); gst(c + 2, noutside); gst(c + 3, 0); }
}

// CoarseTracker.cpp:329-341 per record
__global__ __launch_bounds__(256) void k_ref_accept(int n, RefRecDev R, const float* __restrict__ idepth_stereo, const float* __restrict__ back_uv,
                                                    const uint8_t* __restrict__ status_fwd, const uint8_t* __restrict__ status_back) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float new_idepth = R.flts(RW_CPT2)[i];
  const uint8_t sf = status_fwd[i];
  if (sf == 0 /* IPS_GOOD */) {
    const float ids = idepth_stereo[i];
    const float depth = 1.0f / ids;
    const float u_delta = fabsf((float)R.ints(RW_U)[i] - back_uv[2 * (size_t)i]);
    if (u_delta < 1 && depth > 0 && depth < 50) new_idepth = ids;
  }
  R.flts(RW_NEWID)[i] = new_idepth;
  R.bytes(RW_SFWD)[i] = sf;
  R.bytes(RW_SBACK)[i] = status_back[i];
}

int reserve_records(sdso_ctx* ctx, RefRecSet& S, int n) {
  if (S.d.cap >= n) return SDSO_OK;
  S.d = RefRecDev{nullptr, nullptr, nullptr, 0};   // a group (devbuf.h): the view names no buffer until all three are there
  S.n = 0;
  SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, S.i32, S.f32, S.u8));
  const int cap = n + n / 4 + 64;
  SDSO_HIP(ctx, S.i32.reserve(ctx->stream, (size_t)RW_NINT * cap + 4, (size_t)RW_NINT * cap + 4));
  SDSO_HIP(ctx, S.f32.reserve(ctx->stream, (size_t)RW_NFLT * cap, (size_t)RW_NFLT * cap));
  SDSO_HIP(ctx, S.u8.reserve(ctx->stream, (size_t)RW_NBYTE * cap, (size_t)RW_NBYTE * cap));
  S.d = RefRecDev{S.i32, S.f32, S.u8, cap};
  return SDSO_OK;
}

}  // namespace

extern "C" int sdso_track_make_ref_from_window(sdso_ctx* ctx, int ref_slot, int win, int right_slot, float baseline, const int* point_order,
                                               int n_order, int* n_points_out, int* n_border_out, int* pc_n_out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  // ---- refusals: all before any device work
  BaRefView V;
  int rc = ba_ref_view(ctx, win, &V);
  if (rc) return rc;
  auto il = ctx->pyr.find(V.last_frame_slot), ir = ctx->pyr.find(right_slot);
  SDSO_REQUIRE(ctx, il != ctx->pyr.end(), "the pyramid of the window's newest keyframe has been released");
  SDSO_REQUIRE(ctx, ir != ctx->pyr.end(), "unknown right frame slot");
  SDSO_REQUIRE(ctx, il->second.w[0] == V.w && il->second.h[0] == V.h, "the newest keyframe's pyramid is not of the window's size");
  SDSO_REQUIRE(ctx, ir->second.w[0] == V.w && ir->second.h[0] == V.h, "the right frame's pyramid is not of the window's size");
  SDSO_REQUIRE(ctx, n_order >= 0 && (point_order || n_order == 0), "null point_order");
  if (point_order) {
    std::vector<uint8_t> seen((size_t)std::max(V.np, 1), 0);
    for (int i = 0; i < n_order; i++) {
      const int p = point_order[i];
      SDSO_REQUIRE(ctx, p >= 0 && p < V.np, "point_order entry out of range");
      SDSO_REQUIRE(ctx, !seen[p], "point_order names a point twice");
      seen[p] = 1;
    }
  }
  const int n_items = point_order ? n_order : V.np;
  // ---- STEP1 gather
  if (!ctx->refwin) ctx->refwin = new RefWinState();
  RefRecSet& S = ctx->refwin->sets[ref_slot];
  S.stale = false;
  rc = reserve_records(ctx, S, std::max(n_items, 1));
  if (rc) return rc;
  const RefRecDev R = S.d;
  if (point_order && n_order) SDSO_HIP(ctx, hipMemcpyAsync(R.ints(RW_ORDER), point_order, sizeof(int) * (size_t)n_order, hipMemcpyHostToDevice, ctx->stream));
  launch_timed(ctx, "k_ref_gather", 2, k_ref_gather, dim3(1), dim3(RG_BLOCK), V.dev, (const int*)(point_order ? R.ints(RW_ORDER) : nullptr), n_items, R);
  SDSO_HIP(ctx, hipGetLastError());
  // the one read-back of STEP1: the launches of the chain and of the splat are sized by the number of selected points
  int counts[4] = {0, 0, 0, 0};
  SDSO_HIP(ctx, hipMemcpyAsync(counts, R.counts(), sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = counts[0];
  S.n = n;
  // ---- L->R->L re-observation and the accept rule
  if (n) {
    const float* in[6] = {R.flts(RW_FU), R.flts(RW_FV), R.flts(RW_IMIN), R.flts(RW_IMAX), R.flts(RW_IMIN), R.flts(RW_IMAX)};   // :323-324: the back trace takes the same interval
    MatchChainOut M;
    rc = stereo_match_chain_dev(ctx, V.last_frame_slot, right_slot, V.K, baseline, 1, n, in, counts[1] ? R.bytes(RW_SKIP) : nullptr, &M);
    if (rc) return rc;
    launch_timed(ctx, "k_ref_accept", 2, k_ref_accept, dim3((n + 255) / 256), dim3(256), n, R, M.idepth_stereo, M.back_uv, M.status_fwd, M.status_back);
    SDSO_HIP(ctx, hipGetLastError());
  }
  // ---- STEP1's splat and STEP2-5; installs the reference
  rc = track_make_ref_dev(ctx, ref_slot, V.last_frame_slot, n, R.ints(RW_U), R.ints(RW_V), R.flts(RW_NEWID), R.flts(RW_WGT), pc_n_out, false);
  if (rc) return rc;
  if (n_points_out) *n_points_out = n;
  if (n_border_out) *n_border_out = counts[1] + counts[2];
  return SDSO_OK;
}

extern "C" int sdso_track_get_ref_points(sdso_ctx* ctx, int ref_slot, int* n, int* point, int* u, int* v, float* centerProjectedTo2, uint8_t* status_fwd,
                                         uint8_t* status_back, float* new_idepth, float* weight) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  auto it = ctx->refwin ? ctx->refwin->sets.find(ref_slot) : std::map<int, RefRecSet>::iterator();
  if (!ctx->refwin || it == ctx->refwin->sets.end() || it->second.stale) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_track_make_ref_from_window has run on this reference slot");
  const RefRecSet& S = it->second;
  if (n) *n = S.n;
  if (S.n == 0) return SDSO_OK;
  const RefRecDev& R = S.d;
#define DN(dst, src, T) if (dst) SDSO_HIP(ctx, hipMemcpyAsync((dst), (src), sizeof(T) * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream))
  DN(point, R.ints(RW_POINT), int); DN(u, R.ints(RW_U), int); DN(v, R.ints(RW_V), int);
  DN(centerProjectedTo2, R.flts(RW_CPT2), float); DN(new_idepth, R.flts(RW_NEWID), float); DN(weight, R.flts(RW_WGT), float);
  DN(status_fwd, R.bytes(RW_SFWD), uint8_t); DN(status_back, R.bytes(RW_SBACK), uint8_t);
#undef DN
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}
