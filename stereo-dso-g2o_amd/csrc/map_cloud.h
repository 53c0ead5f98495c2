// KeyFrameDisplay::setFromKF / refreshPC as rules, stated once: the kernels of map.hip evaluate them per lane, csrc/test_map_cloud.cpp checks
// them on a CPU.  Plain C++, no HIP type besides the __host__ __device__ marks.
//
// Reference (src/IOWrapper/Pangolin/KeyFrameDisplay.cpp):
//   :68-83    setFromF     fxi = 1/fx, fyi = 1/fy, cxi = -cx/fx, cyi = -cy/fy, in float
//   :85-165   setFromKF    the four lists of a keyframe as InputPointSparse records; the list decides the status (:115, :129, :144, :158)
//   :174-295  refreshPC    the keep tests (:215-234), the 8 pattern vertices (:237-246) and their colours (:250-289)
// Not here, on purpose (sdso_abi.h, "the device-resident map"): the rand() draws of :240 (sparsity) and :246 (z jitter).  z = depth is
// :246 with every draw at 0.5.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAP_HD __host__ __device__ __forceinline__
#else
#define MAP_HD inline
#endif

namespace sdso {

// ---- one point of the map: 16 floats (64 B).  color[] holds the floats PointHessian::color holds.
constexpr int MAP_REC_FLOATS = 16;
enum { MAP_U = 0, MAP_V = 1, MAP_IDEPTH = 2, MAP_IDH = 3, MAP_BS = 4, MAP_COLOR = 5, MAP_PAD = 13 };   // idepth_hessian, maxRelBaseline
// the status of a record is the list it is in
constexpr int MAP_ST_IMMATURE = 0, MAP_ST_ACTIVE = 1, MAP_ST_MARGINALIZED = 2, MAP_ST_OUT = 3;
constexpr int MAP_PATTERN = 8;

// patternP = staticPattern[8] (src/util/settings.cpp:216), the pattern the library uses everywhere
MAP_HD void map_pattern(int k, int* dx, int* dy) {
  constexpr int8_t P[MAP_PATTERN][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};
  *dx = P[k][0]; *dy = P[k][1];
}

// ---- the record of an immature point (:109-113)
MAP_HD float map_immature_idepth(float idepth_min, float idepth_max) { return (idepth_max + idepth_min) * 0.5f; }
constexpr float MAP_IMMATURE_IDH = 1000.f;   // :112
constexpr float MAP_IMMATURE_BS = 0.f;       // :113

// ---- the keep tests of :215-234, in the reference's order.  0 = kept, else the clause that dropped the point: 1 mode / status, 2 negative
// idepth, 3 scaled variance, 4 absolute variance, 5 baseline.  Every comparison is the reference's, so a NaN operand passes: an immature
// point whose idepth_max is still NaN is kept where its status and relObsBaseline = 0 allow it.
MAP_HD int map_drop_clause(int status, float idepth, float idepth_hessian, float relObsBaseline, int mode, float scaledTH, float absTH, float minBS) {
  if (mode == 1 && status != MAP_ST_ACTIVE && status != MAP_ST_MARGINALIZED) return 1;   // :215
  if (mode == 2 && status != MAP_ST_ACTIVE) return 1;                                    // :216
  if (mode > 2) return 1;                                                                // :217
  if (idepth < 0) return 2;                                                              // :219
  const float depth = 1.0f / idepth;                                                     // :222 (idepth = 0: +inf)
  float depth4 = depth * depth;                                                          // :223
  depth4 *= depth4;                                                                      // :224
  // :225 `1.0f / (idepth_hessian + 0.01)`: 0.01 is a double, so the sum and the quotient are double and the result is rounded to float once
  const float var = (float)(1.0 / ((double)idepth_hessian + 0.01));
  if (var * depth4 > scaledTH) return 3;                                                 // :227
  if (var > absTH) return 4;                                                             // :230
  if (relObsBaseline < minBS) return 5;                                                  // :233
  return 0;
}
MAP_HD bool map_keep(int status, float idepth, float idepth_hessian, float relObsBaseline, int mode, float scaledTH, float absTH, float minBS) {
  return map_drop_clause(status, idepth, idepth_hessian, relObsBaseline, mode, scaledTH, absTH, minBS) == 0;
}

// ---- setFromF's inverse calibration (:77-80), float
struct MapCalib { float fxi, fyi, cxi, cyi; };
MAP_HD MapCalib map_calib(float fx, float fy, float cx, float cy) { return MapCalib{1 / fx, 1 / fy, -cx / fx, -cy / fy}; }

// ---- one pattern vertex (:244-246), float, one rounding per operation (the build has -ffp-contract=off); z = depth
MAP_HD void map_vertex(float u, float v, float depth, int dx, int dy, float fxi, float fyi, float cxi, float cyi, float out[3]) {
  out[0] = ((u + dx) * fxi + cxi) * depth;
  out[1] = ((v + dy) * fyi + cyi) * depth;
  out[2] = depth;
}
// camera frame -> world frame: what Pangolin leaves to the GL matrix of camToWorld.  T = R (9, row-major) then t (3); float, summed left
// to right, one rounding per operation
MAP_HD void map_to_world(const float* T, const float in[3], float out[3]) {
  for (int r = 0; r < 3; r++) out[r] = T[3 * r] * in[0] + T[3 * r + 1] * in[1] + T[3 * r + 2] * in[2] + T[9 + r];
}

// ---- the colour (:250-289).  Mode 0 colours by status; every other mode gives the grey (unsigned char)color[pnt].
// That conversion is truncation for 0 <= c < 256.  Outside it the C++ conversion is undefined; the reference's x86 build converts to int
// (cvttss2si) and keeps the low byte, and the int is INT_MIN — low byte 0 — for a NaN or a value outside int.  The GPU's conversion
// saturates instead, so the cases are spelled out.
MAP_HD uint8_t map_grey(float c) {
  if (!(c >= -2147483648.0f && c < 2147483648.0f)) return 0;
  return (uint8_t)(uint32_t)(int32_t)c;
}
MAP_HD void map_colour(int status, int mode, float c, uint8_t out[3]) {
  if (mode == 0) {
    const bool known = status >= MAP_ST_IMMATURE && status <= MAP_ST_OUT;
    out[0] = (status == MAP_ST_OUT || !known) ? 255 : 0;                                 // :252-281
    out[1] = (status == MAP_ST_IMMATURE || status == MAP_ST_ACTIVE || !known) ? 255 : 0;
    out[2] = (status == MAP_ST_IMMATURE || status == MAP_ST_MARGINALIZED || !known) ? 255 : 0;
    return;
  }
  out[0] = out[1] = out[2] = map_grey(c);                                                // :286-288
}

}  // namespace sdso
