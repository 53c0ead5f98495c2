// CoarseTracker::debugPlotIDepthMap, the statements that decide a byte of the published depth image, stated once: the kernels of
// depth_image.hip evaluate them per lane, csrc/test_depth_image.cpp checks them on a CPU.  Plain C++, no HIP type besides the
// __host__ __device__ marks.
//
// Reference:
//   src/FullSystem/CoarseTracker.cpp:1078-1088   the range: the 5 % and 95 % order statistics of the positive pixels of idepth[0]
//   src/FullSystem/CoarseTracker.cpp:1094-1117   the smoothing of the range against the caller's previous one
//   src/FullSystem/CoarseTracker.cpp:1122-1126   the grey background
//   src/FullSystem/CoarseTracker.cpp:1129-1163   the overlay: one coloured ring per qualifying pixel, in raster order
//   src/util/globalFuncs.h:362-379               makeJet3B
//   src/util/MinimalImage.h:100-112              setPixelCirc
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEPTH_IMG_HD __host__ __device__ __forceinline__
#else
#define DEPTH_IMG_HD inline
#endif

namespace sdso {

struct Rgb8 { uint8_t c[3]; };   // Vec3b

// float -> int as the reference's x86 build converts (cvttss2si): truncation, and INT_MIN for a NaN or a value outside int.  The GPU's
// conversion saturates and gives 0 for a NaN, so the out-of-range cases are spelled out.
DEPTH_IMG_HD int trunc_like_x86(float v) {
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT32_MIN;
  return (int)v;
}

// ---- the range (:1078-1088).  allID holds the pixels with idepth > 0 (a NaN fails the test, +inf passes).  Positive floats order as
// their bit patterns, so the k-th smallest float is the k-th smallest key.
DEPTH_IMG_HD bool depth_in_range_set(float v) { return v > 0; }
DEPTH_IMG_HD uint32_t depth_key(float v) {
  union { float f; uint32_t u; } x;
  x.f = v;
  return x.u;   // sign bit 0 for every member of allID: 31 significant bits
}
DEPTH_IMG_HD float depth_from_key(uint32_t k) {
  union { float f; uint32_t u; } x;
  x.u = k;
  return x.f;
}
// the radix select's digits, most significant first: bits [30:20], [19:9], [8:0]
constexpr int DEPTH_SEL_PASSES = 3;
constexpr int DEPTH_SEL_BINS = 2048;
DEPTH_IMG_HD int depth_sel_shift(int pass) { return pass == 0 ? 20 : pass == 1 ? 9 : 0; }
DEPTH_IMG_HD int depth_sel_bits(int pass) { return pass == 2 ? 9 : 11; }
DEPTH_IMG_HD uint32_t depth_sel_digit(uint32_t key, int pass) { return (key >> depth_sel_shift(pass)) & ((1u << depth_sel_bits(pass)) - 1u); }
DEPTH_IMG_HD uint32_t depth_sel_prefix(uint32_t key, int pass) { return key >> (depth_sel_shift(pass) + depth_sel_bits(pass)); }   // the digits before `pass`
// allID[(int)(n*0.05)] and allID[(int)(n*0.95)], n = size-1: a double product, truncated (:1085-1088).  count >= 1.
DEPTH_IMG_HD int depth_range_rank(int count, int which /* 0: min, 1: max */) {
  const int n = count - 1;
  return (int)(n * (which ? 0.95 : 0.05));
}

// ---- the smoothing (:1090-1117).  have_prev: minID_pt != 0 && maxID_pt != 0; prev[] = {*minID_pt, *maxID_pt}.
// used[] = {minID, maxID} the image is drawn with; with have_prev they are also what the caller's two values become.
DEPTH_IMG_HD void depth_range_smooth(float minID_new, float maxID_new, bool have_prev, const float prev[2], float used[2]) {
  float minID = minID_new, maxID = maxID_new;
  if (have_prev && !(prev[0] < 0 || prev[1] < 0)) {
    const float maxChange = 0.3 * (prev[1] - prev[0]);   // float difference, double product, rounded to float
    if (minID < prev[0] - maxChange) minID = prev[0] - maxChange;
    if (minID > prev[0] + maxChange) minID = prev[0] + maxChange;
    if (maxID < prev[1] - maxChange) maxID = prev[1] - maxChange;
    if (maxID > prev[1] + maxChange) maxID = prev[1] + maxChange;
  }
  used[0] = minID;
  used[1] = maxID;
}

// ---- the background (:1123-1125): int c = I*0.9f; if (c>255) c=255; Vec3b(c,c,c).  A NaN (or a product outside int) gives 0: the
// low byte of the INT_MIN the reference's conversion returns.
DEPTH_IMG_HD uint8_t depth_background(float I) {
  int c = trunc_like_x86(I * 0.9f);
  if (c > 255) c = 255;
  return (uint8_t)c;
}

// ---- makeJet3B (globalFuncs.h:362-379).  A NaN id fails both clamps; the reference's (int)(id*8) is then INT_MIN, no case matches and
// the last line returns white — tested first here, since the GPU's conversion would give 0 and take the icP == 0 case.
DEPTH_IMG_HD Rgb8 make_jet_3b(float id) {
  if (id != id) return {{255, 255, 255}};
  if (id <= 0) return {{128, 0, 0}};
  if (id >= 1) return {{0, 0, 128}};
  const int icP = (int)(id * 8);
  const float ifP = (id * 8) - icP;
  if (icP == 0) return {{(uint8_t)(255 * (0.5 + 0.5 * ifP)), 0, 0}};
  if (icP == 1) return {{255, (uint8_t)(255 * (0.5 * ifP)), 0}};
  if (icP == 2) return {{255, (uint8_t)(255 * (0.5 + 0.5 * ifP)), 0}};
  if (icP == 3) return {{(uint8_t)(255 * (1 - 0.5 * ifP)), 255, (uint8_t)(255 * (0.5 * ifP))}};
  if (icP == 4) return {{(uint8_t)(255 * (0.5 - 0.5 * ifP)), 255, (uint8_t)(255 * (0.5 + 0.5 * ifP))}};
  if (icP == 5) return {{0, (uint8_t)(255 * (1 - 0.5 * ifP)), 255}};
  if (icP == 6) return {{0, (uint8_t)(255 * (0.5 - 0.5 * ifP)), 255}};
  if (icP == 7) return {{0, 0, (uint8_t)(255 * (1 - 0.5 * ifP))}};
  return {{255, 255, 255}};
}

// ---- one source pixel of the overlay (:1131-1160).  bp0 .. bpmw = bp[0], bp[1], bp[-1], bp[wl], bp[-wl]; the sums run in that order
// over the positive values only.  Returns whether the pixel draws a ring; *col its colour.
DEPTH_IMG_HD bool depth_source(float bp0, float bp1, float bpm1, float bpw, float bpmw, float minID, float maxID, Rgb8* col) {
  float sid = 0, nid = 0;
  if (bp0 > 0) { sid += bp0; nid++; }
  if (bp1 > 0) { sid += bp1; nid++; }
  if (bpm1 > 0) { sid += bpm1; nid++; }
  if (bpw > 0) { sid += bpw; nid++; }
  if (bpmw > 0) { sid += bpmw; nid++; }
  if (!(bp0 > 0 || nid >= 3)) return false;
  const float id = ((sid / nid) - minID) / ((maxID - minID));
  *col = make_jet_3b(id);
  return true;
}
// the pixels a source may be: x in [3, w-3), y in [3, h-3) (:1129-1130)
DEPTH_IMG_HD bool depth_source_inside(int x, int y, int w, int h) { return x >= 3 && x < w - 3 && y >= 3 && y < h - 3; }

// ---- setPixelCirc (MinimalImage.h:100-112) writes (u+dx, v+dy) for the 40 offsets of the 7x7 block outside its inner 3x3
constexpr int DEPTH_RING_R = 3;
constexpr int DEPTH_RING_N = 40;
DEPTH_IMG_HD bool depth_ring(int dx, int dy) {
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  return ax <= 3 && ay <= 3 && (ax >= 2 || ay >= 2);
}
// The overlay as a gather.  The reference visits the sources in raster order and later writes win, so output pixel (X, Y) shows the
// LAST source in raster order whose ring covers it: the largest source y, then the largest source x.  Candidate k of an output pixel
// is the source (X - dx, Y - dy) with (dx, dy) = depth_ring_offset(k): k = 0 is the last source in raster order, k = 39 the first.
// The first qualifying candidate decides.  (k counts the ring cells of the 7x7 block row by row, dy = -3 first, dx = -3 first.)
DEPTH_IMG_HD void depth_ring_offset(int k, int* dx, int* dy) {
  // rows dy = -3, -2, 2, 3 hold 7 cells, rows dy = -1, 0, 1 hold 4 (dx = -3, -2, 2, 3)
  int row, col;
  if (k < 14) { row = k / 7; col = k % 7; *dy = row - 3; *dx = col - 3; return; }
  if (k < 26) { row = (k - 14) / 4; col = (k - 14) % 4; *dy = row - 1; *dx = col < 2 ? col - 3 : col; return; }
  row = (k - 26) / 7; col = (k - 26) % 7; *dy = row + 2; *dx = col - 3;
}

}  // namespace sdso
