// The marshalling rules of shim/marshal.h on the CPU alone (no device library: the header calls nothing of it): the immature-point
// columns of sdso_trace_points_t with their gather, the struct they hand out and the scatters; the row-times-column order of the
// 3 x 3 float products; the per-level intrinsics.  tests/test_standins_cpu.py compiles and runs it.
//   test_shim_marshal          prints "marshal ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include "shim/marshal.h"
#include "standins.h"
#include "../../include/sdso_abi.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "test_shim_marshal.cpp:%d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

using sdso_shim::detail::TraceCols;

// ---- columns.  Every member of an ImmaturePoint as one number, in this order:
enum { COLOR = 0, WEIGHTS = 8, GRADH = 16, ENERGYTH = 20, U, V, U_STEREO, V_STEREO, QUALITY, MY_TYPE, IDEPTH_MIN, IDEPTH_MAX, IDEPTH_MIN_STEREO,
       IDEPTH_MAX_STEREO, IDEPTH_STEREO, STATUS, UV0, UV1, INTERVAL, IDX, ID, NMEMBERS };
static FrameHessian host_a, host_b;
static void members(const ImmaturePoint& p, double m[NMEMBERS]) {
  for (int k = 0; k < 8; k++) { m[COLOR + k] = p.color[k]; m[WEIGHTS + k] = p.weights[k]; }
  m[GRADH] = p.gradH(0, 0); m[GRADH + 1] = p.gradH(0, 1); m[GRADH + 2] = p.gradH(1, 0); m[GRADH + 3] = p.gradH(1, 1);
  m[ENERGYTH] = p.energyTH; m[U] = p.u; m[V] = p.v; m[U_STEREO] = p.u_stereo; m[V_STEREO] = p.v_stereo; m[QUALITY] = p.quality; m[MY_TYPE] = p.my_type;
  m[IDEPTH_MIN] = p.idepth_min; m[IDEPTH_MAX] = p.idepth_max; m[IDEPTH_MIN_STEREO] = p.idepth_min_stereo; m[IDEPTH_MAX_STEREO] = p.idepth_max_stereo;
  m[IDEPTH_STEREO] = p.idepth_stereo; m[STATUS] = p.lastTraceStatus; m[UV0] = p.lastTraceUV[0]; m[UV1] = p.lastTraceUV[1];
  m[INTERVAL] = p.lastTracePixelInterval; m[IDX] = p.idxInImmaturePoints; m[ID] = p.id;
}
// member k = base + k, so that every member of every point is a value of its own (the status stays a byte)
static ImmaturePoint make(float base, int status, FrameHessian* host) {
  ImmaturePoint p;
  for (int k = 0; k < 8; k++) { p.color[k] = base + COLOR + k; p.weights[k] = base + WEIGHTS + k; }
  p.gradH(0, 0) = base + GRADH; p.gradH(0, 1) = base + GRADH + 1; p.gradH(1, 0) = base + GRADH + 2; p.gradH(1, 1) = base + GRADH + 3;
  p.energyTH = base + ENERGYTH; p.u = base + U; p.v = base + V; p.u_stereo = base + U_STEREO; p.v_stereo = base + V_STEREO; p.quality = base + QUALITY;
  p.my_type = base + MY_TYPE; p.idepth_min = base + IDEPTH_MIN; p.idepth_max = base + IDEPTH_MAX; p.idepth_min_stereo = base + IDEPTH_MIN_STEREO;
  p.idepth_max_stereo = base + IDEPTH_MAX_STEREO; p.idepth_stereo = base + IDEPTH_STEREO; p.lastTraceStatus = status;
  p.lastTraceUV[0] = base + UV0; p.lastTraceUV[1] = base + UV1; p.lastTracePixelInterval = base + INTERVAL;
  p.idxInImmaturePoints = (int)base + IDX; p.id = (int)base + ID; p.host = host;
  return p;
}
static const std::set<int> TRACED = {QUALITY, STATUS, UV0, UV1, INTERVAL};
static std::set<int> with(std::set<int> s, std::initializer_list<int> more) { s.insert(more); return s; }

// gather src, scatter into fresh points with other values in every member: exactly `written` arrives, the rest stays
template <class Scatter>
static void check_scatter(const TraceCols& C, const std::vector<ImmaturePoint*>& src, const std::set<int>& written, Scatter scatter) {
  for (int i = 0; i < 3; i++) {
    const ImmaturePoint before = make(-1000.f * (i + 1), 77 + i, &host_b);
    ImmaturePoint dst = before;
    scatter(i, &dst);
    double got[NMEMBERS], from[NMEMBERS], kept[NMEMBERS];
    members(dst, got); members(*src[i], from); members(before, kept);
    for (int k = 0; k < NMEMBERS; k++) REQUIRE(got[k] == (written.count(k) ? from[k] : kept[k]));
    REQUIRE(dst.host == &host_b);
  }
}
static void test_columns() {
  ImmaturePoint pts[3] = {make(100, 1, &host_a), make(200, 2, &host_a), make(300, 3, &host_a)};
  std::vector<ImmaturePoint*> src = {&pts[0], &pts[1], &pts[2]};
  {  // traceStereo's form: the stereo pixel, the _stereo interval, and the caller's own idepth_min and idepth_stereo columns bound beside them
    TraceCols C(3);
    C.gather(src, &ImmaturePoint::u_stereo, &ImmaturePoint::v_stereo, &ImmaturePoint::idepth_min_stereo, &ImmaturePoint::idepth_max_stereo);
    std::vector<float> imin(3), ids(3);
    for (int i = 0; i < 3; i++) { imin[i] = pts[i].idepth_min; ids[i] = pts[i].idepth_stereo; }
    const sdso_trace_points_t P = C.abi(imin.data(), ids.data());
    REQUIRE(P.n == 3 && P.u_stereo == C.u.data() && P.v_stereo == C.v.data() && P.idepth_min == imin.data() && P.idepth_min_stereo == C.lo.data());
    REQUIRE(P.idepth_max_stereo == C.hi.data() && P.idepth_stereo == ids.data() && P.color == C.color.data() && P.weights == C.weights.data());
    REQUIRE(P.gradH == C.gradH.data() && P.energyTH == C.energyTH.data() && P.quality == C.quality.data() && P.lastTraceStatus == C.status.data());
    REQUIRE(P.lastTraceUV == C.uv.data() && P.lastTracePixelInterval == C.interval.data());
    REQUIRE(P.idepth_min != nullptr && P.idepth_stereo != nullptr);
    for (int i = 0; i < 3; i++) {
      const ImmaturePoint& p = pts[i];
      REQUIRE(P.u_stereo[i] == p.u_stereo && P.v_stereo[i] == p.v_stereo && P.idepth_min[i] == p.idepth_min && P.idepth_stereo[i] == p.idepth_stereo);
      REQUIRE(P.idepth_min_stereo[i] == p.idepth_min_stereo && P.idepth_max_stereo[i] == p.idepth_max_stereo);
      REQUIRE(P.energyTH[i] == p.energyTH && P.quality[i] == p.quality && P.lastTraceStatus[i] == p.lastTraceStatus && P.lastTracePixelInterval[i] == p.lastTracePixelInterval);
      REQUIRE(P.lastTraceUV[2 * i] == p.lastTraceUV[0] && P.lastTraceUV[2 * i + 1] == p.lastTraceUV[1]);
      for (int k = 0; k < 8; k++) REQUIRE(P.color[i * 8 + k] == p.color[k] && P.weights[i * 8 + k] == p.weights[k]);
      REQUIRE(P.gradH[i * 4] == p.gradH(0, 0) && P.gradH[i * 4 + 1] == p.gradH(0, 1) && P.gradH[i * 4 + 2] == p.gradH(1, 0) && P.gradH[i * 4 + 3] == p.gradH(1, 1));
    }
    check_scatter(C, src, with(TRACED, {IDEPTH_MIN_STEREO, IDEPTH_MAX_STEREO}),
                  [&](int i, ImmaturePoint* p) { C.scatterTraced(i, p, &ImmaturePoint::idepth_min_stereo, &ImmaturePoint::idepth_max_stereo); });
  }
  {  // traceOn's and the resident set's form: u / v, the temporal interval in the struct's one pair of interval columns, the other two unbound
    TraceCols C(3);
    C.gather(src, &ImmaturePoint::u, &ImmaturePoint::v, &ImmaturePoint::idepth_min, &ImmaturePoint::idepth_max);
    const sdso_trace_points_t P = C.abi();
    REQUIRE(P.idepth_min == nullptr && P.idepth_stereo == nullptr);
    REQUIRE(P.n == 3 && P.u_stereo == C.u.data() && P.v_stereo == C.v.data() && P.idepth_min_stereo == C.lo.data() && P.idepth_max_stereo == C.hi.data());
    REQUIRE(P.color == C.color.data() && P.weights == C.weights.data() && P.gradH == C.gradH.data() && P.energyTH == C.energyTH.data() && P.quality == C.quality.data());
    REQUIRE(P.lastTraceStatus == C.status.data() && P.lastTraceUV == C.uv.data() && P.lastTracePixelInterval == C.interval.data());
    for (int i = 0; i < 3; i++)
      REQUIRE(P.u_stereo[i] == pts[i].u && P.v_stereo[i] == pts[i].v && P.idepth_min_stereo[i] == pts[i].idepth_min && P.idepth_max_stereo[i] == pts[i].idepth_max);
    const std::set<int> on = with(TRACED, {IDEPTH_MIN, IDEPTH_MAX});
    check_scatter(C, src, on, [&](int i, ImmaturePoint* p) { C.scatterTraced(i, p, &ImmaturePoint::idepth_min, &ImmaturePoint::idepth_max); });
    std::set<int> fixed = {U, V, ENERGYTH};
    for (int k = 0; k < 20; k++) fixed.insert(COLOR + k);        // color, weights, gradH
    check_scatter(C, src, fixed, [&](int i, ImmaturePoint* p) { C.scatterFixed(i, p); });
  }
}

// ---- row times column: (a b + c d) + e f, not a b + (c d + e f)
static void test_row_times_col() {
  const float h = 5.9604644775390625e-8f;                          // 2^-24: half an ulp of 1
  const float A[9] = {1, 1, 1, 3, -2, 0.5f, 0.25f, 7, -1};
  const float B[9] = {1, 0.1f, 2, h, 0.2f, 3, h, 0.3f, 5};         // column 0 = {1, 2^-24, 2^-24}
  const float left = (A[0] * B[0] + A[1] * B[3]) + A[2] * B[6];    // (1 + 2^-24) + 2^-24: both steps round to even, 1
  const float right = A[0] * B[0] + (A[1] * B[3] + A[2] * B[6]);   // 1 + 2^-23: the next float
  REQUIRE(std::memcmp(&left, &right, sizeof(float)) != 0);
  float out[9];
  sdso_shim::detail::mul33(A, B, out);
  REQUIRE(std::memcmp(&out[0], &left, sizeof(float)) == 0);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const float e = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
      REQUIRE(std::memcmp(&out[i * 3 + j], &e, sizeof(float)) == 0);
    }
  const float v[3] = {1, h, h};
  float o3[3];
  sdso_shim::detail::mul31(A, v, o3);
  REQUIRE(std::memcmp(&o3[0], &left, sizeof(float)) == 0);
  for (int i = 0; i < 3; i++) {
    const float e = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
    REQUIRE(std::memcmp(&o3[i], &e, sizeof(float)) == 0);
  }
}

// ---- per-level intrinsics: the KITTI-shaped calibration of tests/synth.py (kitti_calib) at 1232 x 368, 6 levels, in the two
// arithmetic types the rule is written for.  Expected: the three lines of the two makeK bodies.
template <class S>
static void test_levels() {
  const int W = 1232, H = 368, L = 6;
  const float f = (float)(718.856 * (W / 1241.0));
  CalibHessian calib(f, f, (float)(W / 2.0 - 0.5 + 3.2), (float)(H / 2.0 - 0.5 - 2.9));
  int w[L], h[L], ew[L], eh[L];
  S fx[L], fy[L], cx[L], cy[L], efx[L], efy[L], ecx[L], ecy[L];
  sdso_shim::detail::levelIntrinsics(&calib, L, W, H, w, h, fx, fy, cx, cy);
  ew[0] = W; eh[0] = H;
  efx[0] = calib.fxl(); efy[0] = calib.fyl(); ecx[0] = calib.cxl(); ecy[0] = calib.cyl();
  for (int l = 1; l < L; ++l) {
    ew[l] = W >> l; eh[l] = H >> l;
    efx[l] = efx[l - 1] * 0.5; efy[l] = efy[l - 1] * 0.5;
    ecx[l] = (ecx[0] + 0.5) / ((int)1 << l) - 0.5; ecy[l] = (ecy[0] + 0.5) / ((int)1 << l) - 0.5;
  }
  REQUIRE(std::memcmp(w, ew, sizeof(w)) == 0 && std::memcmp(h, eh, sizeof(h)) == 0);
  REQUIRE(std::memcmp(fx, efx, sizeof(fx)) == 0 && std::memcmp(fy, efy, sizeof(fy)) == 0);
  REQUIRE(std::memcmp(cx, ecx, sizeof(cx)) == 0 && std::memcmp(cy, ecy, sizeof(cy)) == 0);
  REQUIRE(w[5] == 38 && h[5] == 11 && fx[0] == (S)f && fx[5] == (S)f / 32 && cx[0] != cy[0]);
}

// ---- the calibration as the reference declares it: accessors that are not const and return references (FullSystem/HessianBlocks.h:307-310).
// The stand-in's are const, so only this type shows that the helpers take the calibration as the callers hold it.
struct ReferenceShapedCalib {
  float value_scaledf[4];
  float& fxl() { return value_scaledf[0]; }
  float& fyl() { return value_scaledf[1]; }
  float& cxl() { return value_scaledf[2]; }
  float& cyl() { return value_scaledf[3]; }
};
static void test_reference_shaped_calib() {
  ReferenceShapedCalib c{{700.5f, 701.5f, 618.7f, 180.6f}};
  float K4[4];
  sdso_shim::detail::calibK4(c, K4);
  REQUIRE(std::memcmp(K4, c.value_scaledf, sizeof(K4)) == 0);
  int w[2], h[2];
  float fx[2], fy[2], cx[2], cy[2];
  sdso_shim::detail::levelIntrinsics(&c, 2, 1232, 368, w, h, fx, fy, cx, cy);
  REQUIRE(fx[0] == 700.5f && fy[1] == 701.5f * 0.5f && cx[0] == 618.7f && cy[0] == 180.6f && w[1] == 616 && h[1] == 184);
}

int main() {
  test_reference_shaped_calib();
  test_columns();
  test_row_times_col();
  test_levels<double>();
  test_levels<float>();
  std::printf("marshal ok\n");
  return 0;
}
