// CoarseTracker::debugPlotIDepthMap / debugPlotIDepthMapFloat on gfx950: the keyframe's published depth images from the level-0 map a
// template keeps under sdso_track_keep_depth_map (coarse_depth.hip).  Every statement that decides a byte is in depth_image.h.
//
// Reference (src/FullSystem/CoarseTracker.cpp):
//   :1078-1088  the range    k_di_hist + k_di_pick, three times: a radix select of allID[(int)(n*0.05)] and allID[(int)(n*0.95)] over the
//                            bit patterns of the positive pixels, 11 + 11 + 9 bits.  Integer atomics only: the histograms, and so the
//                            two values, do not depend on the order of arrival.  No sort.
//   :1094-1117  smoothing    one thread of the last k_di_pick
//   :1122-1163  the image    k_di_image: background and overlay in one pass.  The reference scatters a 40-pixel ring per source in
//                            raster order, later writes winning; here every output pixel looks its 40 possible sources up, last one
//                            first, in an LDS tile that holds each source's test and colour once.  No atomics on the image, no second
//                            image.
//   :1178-1188  the float image is the kept map itself.
#include "sdso_internal.h"
#include "depth_image.h"
#include <algorithm>
#include <cstring>

using namespace sdso;

namespace {

// the work area of one call in ctx->scratch, zeroed by one memset ahead of the chain
struct DiWork {
  unsigned hist[DEPTH_SEL_PASSES][2][DEPTH_SEL_BINS];   // pass 0 fills [0][0] only: both ranks start from the same histogram
  unsigned prefix[2];                                    // the digits found so far of allID[rank_min], allID[rank_max]
  unsigned rank[2];                                      // the rank that remains inside the prefix
  int count;                                             // allID.size()
};
// the 16-byte record behind the kept map (depth_map_layout): what the call returns besides the images
struct DiRecord { float used[2]; int count, circles; };

constexpr int DI_HIST_MAX_BLOCKS = 256;

__global__ __launch_bounds__(256) void k_di_hist(const float* __restrict__ map, int npx, int pass, DiWork* __restrict__ W) {
  __shared__ unsigned s_h[2][DEPTH_SEL_BINS];
  for (int k = threadIdx.x; k < 2 * DEPTH_SEL_BINS; k += blockDim.x) (&s_h[0][0])[k] = 0;
  const unsigned p0 = W->prefix[0], p1 = W->prefix[1];
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
    const float v = map[i];
    if (!depth_in_range_set(v)) continue;
    const uint32_t key = depth_key(v), d = depth_sel_digit(key, pass);
    if (pass == 0) { atomicAdd(&s_h[0][d], 1u); continue; }
    const uint32_t pre = depth_sel_prefix(key, pass);
    if (pre == p0) atomicAdd(&s_h[0][d], 1u);
    if (pre == p1) atomicAdd(&s_h[1][d], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * DEPTH_SEL_BINS; k += blockDim.x) {
    const unsigned c = (&s_h[0][0])[k];
    if (c) atomicAdd(&W->hist[pass][0][0] + k, c);
  }
}

// One workgroup: the bin of each of the two ranks in this pass's histogram.  The last pass ends with the smoothing and the record.
__global__ __launch_bounds__(256) void k_di_pick(int pass, DiWork* __restrict__ W, int have_prev, float prev0, float prev1, DiRecord* __restrict__ rec) {
  constexpr int PER = DEPTH_SEL_BINS / 256;
  __shared__ unsigned s[256];
  const int tid = threadIdx.x;
  for (int t = 0; t < 2; t++) {
    const unsigned* H = W->hist[pass][pass == 0 ? 0 : t];
    unsigned loc[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) { loc[j] = H[tid * PER + j]; sum += loc[j]; }
    unsigned rank = W->rank[t];
    const unsigned prefix = W->prefix[t];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned add = tid >= o ? s[tid - o] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    const unsigned incl = s[tid], total = s[255];
    __syncthreads();
    if (pass == 0) {
      if (tid == 0 && t == 0) W->count = (int)total;
      rank = total ? (unsigned)depth_range_rank((int)total, t) : 0u;   // the index arithmetic of :1085-1088, in double
    }
    unsigned excl = incl - sum;
    if (total && rank >= excl && rank < incl) {   // exactly one thread
#pragma unroll
      for (int j = 0; j < PER; j++) {
        if (rank < excl + loc[j]) {
          W->prefix[t] = (prefix << depth_sel_bits(pass)) | (unsigned)(tid * PER + j);
          W->rank[t] = rank - excl;
          break;
        }
        excl += loc[j];
      }
    }
  }
  if (pass != DEPTH_SEL_PASSES - 1) return;
  __syncthreads();
  if (tid == 0) {
    const int count = W->count;
    const float prev[2] = {prev0, prev1};
    float used[2] = {prev0, prev1};   // no positive pixel: the range is left as it came
    if (count > 0) depth_range_smooth(depth_from_key(W->prefix[0]), depth_from_key(W->prefix[1]), have_prev != 0, prev, used);
    rec->used[0] = used[0]; rec->used[1] = used[1];
    rec->count = count; rec->circles = 0;
  }
}

// The image.  A workgroup draws DI_TX x DI_TY output pixels, one wave per row at a time: consecutive lanes read consecutive LDS words.
//   s_map  the map under the tile with a halo of 4 (a source lies up to 3 pixels away and reads its 4 neighbours), -1 outside the image
//   s_src  per possible source (halo 3): bit 31 = it draws a ring, bits 0..23 = its colour; 0 outside [3,w-3) x [3,h-3)
constexpr int DI_TX = 64, DI_TY = 16;
constexpr int DI_MW = DI_TX + 2 * (DEPTH_RING_R + 1), DI_MH = DI_TY + 2 * (DEPTH_RING_R + 1);
constexpr int DI_SW = DI_TX + 2 * DEPTH_RING_R, DI_SH = DI_TY + 2 * DEPTH_RING_R;

__global__ __launch_bounds__(256) void k_di_image(const float* __restrict__ map, const float4* __restrict__ img, int w, int h, DiRecord* __restrict__ rec,
                                                  uint8_t* __restrict__ rgb) {
  __shared__ float s_map[DI_MH * DI_MW];
  __shared__ uint32_t s_src[DI_SH * DI_SW];
  const int tid = threadIdx.x, x0 = blockIdx.x * DI_TX, y0 = blockIdx.y * DI_TY;
  for (int i = tid; i < DI_MH * DI_MW; i += 256) {
    const int mx = x0 - (DEPTH_RING_R + 1) + i % DI_MW, my = y0 - (DEPTH_RING_R + 1) + i / DI_MW;
    s_map[i] = (mx >= 0 && mx < w && my >= 0 && my < h) ? map[(size_t)my * w + mx] : -1.f;
  }
  const float minID = rec->used[0], maxID = rec->used[1];
  const bool any = rec->count > 0;
  __syncthreads();
  int drew = 0;
  for (int i0 = 0; i0 < DI_SH * DI_SW; i0 += 256) {
    const int i = i0 + tid;
    bool own = false;
    if (i < DI_SH * DI_SW) {
      const int lx = i % DI_SW, ly = i / DI_SW;
      const int sx = x0 - DEPTH_RING_R + lx, sy = y0 - DEPTH_RING_R + ly;
      uint32_t val = 0;
      if (any && depth_source_inside(sx, sy, w, h)) {
        const float* m = &s_map[(ly + 1) * DI_MW + lx + 1];
        Rgb8 col;
        if (depth_source(m[0], m[1], m[-1], m[DI_MW], m[-DI_MW], minID, maxID, &col)) {
          val = 0x80000000u | col.c[0] | ((uint32_t)col.c[1] << 8) | ((uint32_t)col.c[2] << 16);
          own = lx >= DEPTH_RING_R && lx < DEPTH_RING_R + DI_TX && ly >= DEPTH_RING_R && ly < DEPTH_RING_R + DI_TY;   // counted by the tile it lies in
        }
      }
      s_src[i] = val;
    }
    drew += __popcll(__ballot(own));
  }
  if ((tid & 63) == 0 && drew) atomicAdd(&rec->circles, drew);
  __syncthreads();
  const int tx = tid & 63;
#pragma unroll
  for (int r = 0; r < DI_TY / 4; r++) {
    const int ty = (tid >> 6) + 4 * r;
    const int X = x0 + tx, Y = y0 + ty;
    if (X >= w || Y >= h) continue;
    const size_t o = (size_t)Y * w + X;
    const uint8_t bg = depth_background(img[o].x);
    uint32_t out = bg | ((uint32_t)bg << 8) | ((uint32_t)bg << 16);
#pragma unroll
    for (int k = 0; k < DEPTH_RING_N; k++) {
      int dx, dy;
      depth_ring_offset(k, &dx, &dy);
      const uint32_t v = s_src[(ty - dy + DEPTH_RING_R) * DI_SW + (tx - dx + DEPTH_RING_R)];
      if (v & 0x80000000u) { out = v; break; }
    }
    rgb[3 * o + 0] = (uint8_t)out; rgb[3 * o + 1] = (uint8_t)(out >> 8); rgb[3 * o + 2] = (uint8_t)(out >> 16);
  }
}

}  // namespace

extern "C" int sdso_track_depth_image(sdso_ctx* ctx, int ref_slot, int frame_slot, float* minID_pt, float* maxID_pt, uint8_t* rgb, float* idepth,
                                      int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  // ---- refusals: all before any device work
  auto ir = ctx->refs.find(ref_slot);
  SDSO_REQUIRE(ctx, ir != ctx->refs.end(), "unknown reference slot");
  SDSO_REQUIRE(ctx, (minID_pt == nullptr) == (maxID_pt == nullptr), "minID_pt / maxID_pt: both or neither");
  PyramidDev* P = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &P));
  RefDev& R = ir->second;
  if (!R.map_ok) return sdso::fail(ctx, SDSO_ERR_STATE, "the reference slot keeps no level-0 map (sdso_track_keep_depth_map was off when it was built, or sdso_track_set_ref installed it)");
  const int w = R.dmap_w, h = R.dmap_h, npx = w * h;
  SDSO_REQUIRE(ctx, P->w[0] == w && P->h[0] == h, "the frame differs in size from the kept map");
  // ---- the chain
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const DepthMapLayout L = depth_map_layout(w, h);
  SDSO_TRY(ensure_scratch(ctx, sizeof(DiWork)));
  SDSO_TRY(ensure_pinned(ctx, L.end));
  DiWork* W = (DiWork*)ctx->scratch;
  const float* map = (const float*)R.dmap;
  DiRecord* rec = (DiRecord*)(R.dmap + L.rec);
  const int have_prev = minID_pt != nullptr;
  const float prev0 = have_prev ? *minID_pt : 0.f, prev1 = have_prev ? *maxID_pt : 0.f;
  SDSO_HIP(ctx, hipMemsetAsync(W, 0, sizeof(DiWork), ctx->stream));
  const int hb = std::max(1, std::min(DI_HIST_MAX_BLOCKS, (npx + 1023) / 1024));
  for (int pass = 0; pass < DEPTH_SEL_PASSES; pass++) {
    launch_timed(ctx, "k_di_hist", 2, k_di_hist, dim3(hb), dim3(256), map, npx, pass, W);
    launch_timed(ctx, "k_di_pick", 2, k_di_pick, dim3(1), dim3(256), pass, W, have_prev, prev0, prev1, rec);
  }
  launch_timed(ctx, "k_di_image", 2, k_di_image, dim3((w + DI_TX - 1) / DI_TX, (h + DI_TY - 1) / DI_TY), dim3(256), map, (const float4*)P->d[0], w, h, rec,
               (uint8_t*)(R.dmap + L.rgb));
  SDSO_HIP(ctx, hipGetLastError());
  R.image_ok = true;
  // ---- one copy: the record with whichever images were asked for, contiguous in the kept block
  const size_t a = idepth ? 0 : L.rec, b = rgb ? L.end : L.rgb;
  char* host = (char*)ctx->pinned;
  SDSO_HIP(ctx, hipMemcpyAsync(host, R.dmap + a, b - a, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  DiRecord out;
  memcpy(&out, host + (L.rec - a), sizeof(out));
  if (idepth) memcpy(idepth, host, L.rec);
  if (rgb) memcpy(rgb, host + (L.rgb - a), L.end - L.rgb);
  if (counts) { counts[0] = out.count; counts[1] = out.circles; }
  if (have_prev && out.count > 0) { *minID_pt = out.used[0]; *maxID_pt = out.used[1]; }
  return SDSO_OK;
}

extern "C" int sdso_track_depth_image_dev(sdso_ctx* ctx, int ref_slot, void** rgb_dev, void** idepth_dev, int* w, int* h) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, rgb_dev && idepth_dev && w && h, "null argument");
  auto ir = ctx->refs.find(ref_slot);
  SDSO_REQUIRE(ctx, ir != ctx->refs.end(), "unknown reference slot");
  const RefDev& R = ir->second;
  if (!R.map_ok || !R.image_ok) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_track_depth_image has run on this reference slot's template");
  *rgb_dev = R.dmap + depth_map_layout(R.dmap_w, R.dmap_h).rgb;
  *idepth_dev = R.dmap;
  *w = R.dmap_w; *h = R.dmap_h;
  return SDSO_OK;
}
