// The marshalling rules more than one part follows, each stated once: the shim's tests compare its route with the ABI's exactly, so a rule
// fixes an ORDER (of members, of a float sum) as well as a layout.  Nothing here calls into the library.
#pragma once
#include <type_traits>
#include <vector>
#include "../../../include/sdso_abi.h"
namespace sdso_shim {
// ---- SE3 / AffLight marshalling (Sophus::SE3d API: rotationMatrix()(i,j), translation()[i], ctor(R, t))
template <class SE3T> inline sdso_se3_t toAbi(const SE3T& T) {
  sdso_se3_t o;
  const auto R = T.rotationMatrix();
  const auto t = T.translation();
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o.R[i * 3 + j] = R(i, j); o.t[i] = t[i]; }
  return o;
}
template <class SE3T, class Mat33T, class Vec3T> inline SE3T fromAbi(const sdso_se3_t& a) {
  Mat33T R;
  Vec3T t;
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R(i, j) = a.R[i * 3 + j]; t[i] = a.t[i]; }
  return SE3T(R, t);
}
namespace detail {
// a vector / an n x m matrix of the reference (Eigen: [i] / (i, j)) from a row-major buffer of the ABI
template <class V> inline void fill(V& v, const double* src, int n) { for (int i = 0; i < n; i++) v[i] = src[i]; }
template <class M> inline void fill(M& H, const double* src, int n, int m) { for (int i = 0; i < n; i++) for (int j = 0; j < m; j++) H(i, j) = src[(size_t)i * m + j]; }
// 3 x 3 float products (row-major float[9]) as the reference's Eigen expressions round them: (a0 b0 + a1 b1) + a2 b2; toFloat9 = .cast<float>()
inline float rowTimesCol(const float* row, const float* col, int stride) { return (row[0] * col[0] + row[1] * col[stride]) + row[2] * col[2 * stride]; }
inline void mul33(const float A[9], const float B[9], float out[9]) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) out[i * 3 + j] = rowTimesCol(A + i * 3, B + j, 3); }
inline void mul31(const float A[9], const float v[3], float out[3]) { for (int i = 0; i < 3; i++) out[i] = rowTimesCol(A + i * 3, v, 1); }
template <class M> inline void toFloat9(const M& m, float out[9]) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) out[i * 3 + j] = (float)m(i, j); }
// m.inverse() where the type has one (Eigen); else cofactors times 1 / det, in the matrix's own scalar type
template <class M> inline auto inverse33(const M& m, int) -> decltype(m.inverse()) { return m.inverse(); }
template <class M> inline M inverse33(const M& m, long) {
  using S = typename std::decay<decltype(m(0, 0))>::type;
  M r;
  const S c00 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), c10 = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), c20 = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0);
  const S id = S(1) / (c00 * m(0, 0) + c10 * m(0, 1) + c20 * m(0, 2));
  r(0, 0) = c00 * id; r(1, 0) = c10 * id; r(2, 0) = c20 * id;
  r(0, 1) = (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * id; r(1, 1) = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * id; r(2, 1) = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * id;
  r(0, 2) = (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * id; r(1, 2) = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * id; r(2, 2) = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * id;
  return r;
}
// K4 = {fxl, fyl, cxl, cyl} of a CalibHessian (its accessors are not const in the reference), and the 3 x 3 K of a pinhole
template <class CalibHessianT> inline void calibK4(CalibHessianT& c, float K4[4]) { K4[0] = c.fxl(); K4[1] = c.fyl(); K4[2] = c.cxl(); K4[3] = c.cyl(); }
template <class Mat33T, class S> inline void pinholeK(Mat33T& K, S fx, S fy, S cx, S cy) {
  using E = typename std::decay<decltype(K(0, 0))>::type;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K(i, j) = i == j ? E(1) : E(0);
  K(0, 0) = fx; K(1, 1) = fy; K(0, 2) = cx; K(1, 2) = cy;
}
// makeK's per-level intrinsics (CoarseTracker.cpp:108-136, :1374-1390): double arithmetic rounded into the caller's storage type S
template <class CalibHessianT, class S>
inline void levelIntrinsics(CalibHessianT* HCalib, int levels, int w0, int h0, int* w, int* h, S* fx, S* fy, S* cx, S* cy) {
  w[0] = w0; h[0] = h0;
  fx[0] = HCalib->fxl(); fy[0] = HCalib->fyl(); cx[0] = HCalib->cxl(); cy[0] = HCalib->cyl();
  for (int l = 1; l < levels; ++l) {
    w[l] = w0 >> l; h[l] = h0 >> l;
    fx[l] = fx[l - 1] * 0.5; fy[l] = fy[l - 1] * 0.5;
    cx[l] = (cx[0] + 0.5) / ((int)1 << l) - 0.5;
    cy[l] = (cy[0] + 0.5) / ((int)1 << l) - 0.5;
  }
}
// n ImmaturePoints as the columns of sdso_trace_points_t (ImmaturePoint.h:60-102).  The struct has ONE pair of interval columns, lo / hi here:
// the caller names the members that travel as the pixel and as the interval.  idepth_min and idepth_stereo are traceStereo's alone, which
// brings its own two columns to abi(); everyone else hands them out as nullptr.  my_type is no column of the struct and stays with the callers.
struct TraceCols {
  const int n;
  std::vector<float> u, v, lo, hi, color, weights, gradH, energyTH, quality, uv, interval;
  std::vector<uint8_t> status;
  explicit TraceCols(int n_) : n(n_), u(n_), v(n_), lo(n_), hi(n_), color(n_ * 8), weights(n_ * 8), gradH(n_ * 4), energyTH(n_), quality(n_), uv(n_ * 2), interval(n_), status(n_) {}
  sdso_trace_points_t abi(float* idepth_min = nullptr, float* idepth_stereo = nullptr) {
    return sdso_trace_points_t{n, u.data(), v.data(), idepth_min, lo.data(), hi.data(), idepth_stereo, color.data(), weights.data(), gradH.data(), energyTH.data(),
                               quality.data(), status.data(), uv.data(), interval.data()};
  }
  template <class P, class S> void gather(const std::vector<P*>& pts, S P::*pu, S P::*pv, S P::*plo, S P::*phi) {
    for (int i = 0; i < n; i++) {
      const P* p = pts[i];
      u[i] = p->*pu; v[i] = p->*pv; lo[i] = p->*plo; hi[i] = p->*phi;
      energyTH[i] = p->energyTH; quality[i] = p->quality; status[i] = (uint8_t)p->lastTraceStatus;
      uv[2 * i] = p->lastTraceUV[0]; uv[2 * i + 1] = p->lastTraceUV[1]; interval[i] = p->lastTracePixelInterval;
      for (int k = 0; k < 8; k++) { color[i * 8 + k] = p->color[k]; weights[i * 8 + k] = p->weights[k]; }
      gradH[i * 4 + 0] = p->gradH(0, 0); gradH[i * 4 + 1] = p->gradH(0, 1); gradH[i * 4 + 2] = p->gradH(1, 0); gradH[i * 4 + 3] = p->gradH(1, 1);
    }
  }
  // point i -> *p: what a trace changes (the interval into the two named members, quality, the lastTrace members) ...
  template <class P, class S> void scatterTraced(int i, P* p, S P::*plo, S P::*phi) const {
    p->*plo = lo[i]; p->*phi = hi[i]; p->quality = quality[i];
    p->lastTraceStatus = static_cast<decltype(p->lastTraceStatus)>(status[i]);
    p->lastTraceUV[0] = uv[2 * i]; p->lastTraceUV[1] = uv[2 * i + 1]; p->lastTracePixelInterval = interval[i];
  }
  // ... and what it leaves alone, for an object made from the device-resident set
  template <class P> void scatterFixed(int i, P* p) const {
    p->u = u[i]; p->v = v[i]; p->energyTH = energyTH[i];
    for (int k = 0; k < 8; k++) { p->color[k] = color[i * 8 + k]; p->weights[k] = weights[i * 8 + k]; }
    p->gradH(0, 0) = gradH[i * 4 + 0]; p->gradH(0, 1) = gradH[i * 4 + 1]; p->gradH(1, 0) = gradH[i * 4 + 2]; p->gradH(1, 1) = gradH[i * 4 + 3];
  }
};
}  // namespace detail
}  // namespace sdso_shim
