// The epipolar search of ImmaturePoint::traceStereo (ImmaturePoint.cpp:94-451) and ImmaturePoint::traceOn (:459-828), stated once:
//   trace_line         the search line: interval ends, border tests, step, errorInPixel, numSteps   (:118-260 / :480-657)
//   trace_step_energy  the energy of one discrete step                                              (:262-285 / :659-683)
//   trace_first_min    the first minimum over the steps and the second best outside its radius      (:286-305 / :684-702)
//   trace_gn_terms / trace_gn_advance   one pattern pixel / one iteration of the DSO-native sub-pixel Gauss-Newton (:707-769)
//   trace_interval     the new idepth interval around the refined position                          (:424-436 / :798-810)
// with TraceDev (a batch of points), the constants, the status enum and the writer of a fresh ImmaturePoint's members.  The reference
// writes all of this twice; k_trace_stereo_blk (stereo_trace.hip: a workgroup per 16 points) and trace_on_point (one wave per point) differ
// only in their lane layout, in where pr / Kt come from (a camera pair / a hostToFrame geometry) and in the pattern offsets and affine
// pair of a sample (TracePatStereo / TracePatOn).  No helper has a lane test or a store, and none knows its caller.  Every expression
// keeps the reference's association (the library is compiled without FP contraction): the results are bit-identical to the CPU path.
// Included by stereo.hip alone (c_pat is a definition).
#pragma once
#include "sdso_internal.h"

namespace sdso {

__constant__ int c_pat[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};
constexpr float kMaxPixSearch = 0.027f, kTraceStepsize = 1.0f, kTraceGNThreshold = 0.1f, kTraceExtraSlack = 1.2f,
                kTraceSlackInterval = 1.5f, kTraceMinImprovement = 2.f, kOutlierTH = 144.f;
constexpr int kTraceGNIterations = 3, kMinTraceTestRadius = 2;
enum { IPS_GOOD = 0, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED };

struct TraceDev {
  int n, w, h, mode_right;
  float fx, fy, cx, cy, baseline;
  const float4* img;
  const float* plane;   // level-0 intensities only (discrete search)
  float *u_stereo, *v_stereo, *idepth_min, *idepth_min_stereo, *idepth_max_stereo, *idepth_stereo;
  const float *color, *weights, *gradH, *energyTH;
  float* quality; uint8_t* lastTraceStatus; float* lastTraceUV; float* lastTracePixelInterval;
  uint8_t* status;
  const uint8_t* skip;   // optional: 1 = leave the point alone (status 255)
};

// The constructor (ImmaturePoint.cpp:33-62) and the searches dereference the 3x3 neighbourhood of every pattern pixel unchecked: the
// entry points refuse a point elsewhere, the chains give it no trace.
__host__ __device__ inline bool trace_pattern_readable(float u, float v, int w, int h) { return u >= 2 && v >= 2 && u < w - 3 && v < h - 3; }
// where a point that takes no trace is parked, both coordinates: a harmless pixel, so that the constructor kernel reads valid memory
constexpr float kTraceParkedPixel = 8.f;

// the members of a fresh ImmaturePoint (ImmaturePoint.cpp:34-38) at (u, v), with the interval its maker gives it
__device__ __forceinline__ void fresh_point(const TraceDev& T, int j, float u, float v, float idepth_min, float imin_stereo, float imax_stereo) {
  T.u_stereo[j] = u; T.v_stereo[j] = v;
  T.idepth_min[j] = idepth_min;
  T.idepth_min_stereo[j] = imin_stereo; T.idepth_max_stereo[j] = imax_stereo;
  T.idepth_stereo[j] = 0.f; T.quality[j] = 10000.f; T.lastTraceStatus[j] = IPS_UNINITIALIZED;
  T.lastTraceUV[2 * j] = 0.f; T.lastTraceUV[2 * j + 1] = 0.f; T.lastTracePixelInterval[j] = 0.f;
}

// getInterpolatedElement33BiLin (src/util/globalFuncs.h:160-184)
__device__ __forceinline__ float3 interp33BiLin(const float4* __restrict__ img, float x, float y, int width) {
  const int ix = (int)x, iy = (int)y;
  const float4* bp = img + ix + iy * width;
  const float tl = bp[0].x, tr = bp[1].x, bl = bp[width].x, br = bp[width + 1].x;
  const float dx = x - ix, dy = y - iy;
  const float topInt = dx * tr + (1 - dx) * tl;
  const float botInt = dx * br + (1 - dx) * bl;
  const float leftInt = dy * bl + (1 - dy) * tl;
  const float rightInt = dy * br + (1 - dy) * tr;
  return make_float3(dx * rightInt + (1 - dx) * leftInt, rightInt - leftInt, botInt - topInt);
}

// ---- the search line
struct TraceLine {
  float uMin, vMin, uMax, vMax, dist;   // the interval's ends as projected, before the clamp to maxPixSearch: also set with SKIPPED and BADCONDITION
  float dx, dy, errorInPixel, ptx0, pty0;
  int numSteps;
};
constexpr int kTraceSearch = -1;   // trace_line: the point goes on to the search
// pr = K R K^-1 (u, v, 1), Kt = K t; idepth_min is the value of the `idepth_min < 0` rule.  Returns kTraceSearch or the
// status that ends the point (IPS_OOB, IPS_SKIPPED, IPS_BADCONDITION); what the caller writes with that status is its own affair.
__device__ __forceinline__ int trace_line(const float (&pr)[3], const float (&Kt)[3], const float idepth_min, const float idepth_min_stereo,
                                          const float idepth_max_stereo, const float* gradH, const int wG0, const int hG0, TraceLine& L) {
  float ptpMin[3];
#pragma unroll
  for (int k = 0; k < 3; k++) ptpMin[k] = pr[k] + Kt[k] * idepth_min_stereo;
  const float uMin = L.uMin = ptpMin[0] / ptpMin[2];
  const float vMin = L.vMin = ptpMin[1] / ptpMin[2];
  if (!(uMin > 4 && vMin > 4 && uMin < wG0 - 5 && vMin < hG0 - 5)) return IPS_OOB;
  float dist, uMax, vMax, ptpMax[3];
  const float maxPixSearch = (wG0 + hG0) * kMaxPixSearch;
  const bool finiteMax = isfinite(idepth_max_stereo);
  if (finiteMax) {
#pragma unroll
    for (int k = 0; k < 3; k++) ptpMax[k] = pr[k] + Kt[k] * idepth_max_stereo;
    uMax = ptpMax[0] / ptpMax[2];
    vMax = ptpMax[1] / ptpMax[2];
    if (!(uMax > 4 && vMax > 4 && uMax < wG0 - 5 && vMax < hG0 - 5)) return IPS_OOB;
    dist = (uMin - uMax) * (uMin - uMax) + (vMin - vMax) * (vMin - vMax);
    dist = sqrtf(dist);
    L.uMax = uMax; L.vMax = vMax; L.dist = dist;
    if (dist < kTraceSlackInterval) return IPS_SKIPPED;
  } else {
    dist = maxPixSearch;
#pragma unroll
    for (int k = 0; k < 3; k++) ptpMax[k] = pr[k] + Kt[k] * 0.01f;
    uMax = ptpMax[0] / ptpMax[2];
    vMax = ptpMax[1] / ptpMax[2];
    const float ddx = uMax - uMin;
    const float ddy = vMax - vMin;
    const float d = 1.0f / sqrtf(ddx * ddx + ddy * ddy);
    uMax = uMin + dist * ddx * d;
    vMax = vMin + dist * ddy * d;
    if (!(uMax > 4 && vMax > 4 && uMax < wG0 - 5 && vMax < hG0 - 5)) return IPS_OOB;
    L.uMax = uMax; L.vMax = vMax; L.dist = dist;
  }
  if (!(idepth_min < 0 || (ptpMin[2] > 0.75 && ptpMin[2] < 1.5))) return IPS_OOB;
  float dx = kTraceStepsize * (uMax - uMin);
  float dy = kTraceStepsize * (vMax - vMin);
  const float a = (dx * gradH[0] + dy * gradH[2]) * dx + (dx * gradH[1] + dy * gradH[3]) * dy;
  const float b = (dy * gradH[0] + (-dx) * gradH[2]) * dy + (dy * gradH[1] + (-dx) * gradH[3]) * (-dx);
  float errorInPixel = 0.2f + 0.2f * (a + b) / a;
  if (errorInPixel * kTraceMinImprovement > dist && finiteMax) return IPS_BADCONDITION;
  if (errorInPixel > 10) errorInPixel = 10;
  dx /= dist;
  dy /= dist;
  if (dist > maxPixSearch) {
    uMax = uMin + maxPixSearch * dx;
    vMax = vMin + maxPixSearch * dy;
    dist = maxPixSearch;
  }
  int numSteps = 1.9999f + dist / kTraceStepsize;
  const float randShift = uMin * 1000 - floorf(uMin * 1000);
  L.ptx0 = uMin - randShift * dx;
  L.pty0 = vMin - randShift * dy;
  if (!isfinite(dx) || !isfinite(dy)) return IPS_OOB;
  if (numSteps >= 100) numSteps = 99;
  L.dx = dx; L.dy = dy; L.errorInPixel = errorInPixel; L.numSteps = numSteps;
  return kTraceSearch;
}

// ---- where a sample's pattern offsets and affine pair come from
struct TracePatStereo {   // traceStereo: the pattern itself and the identity pair, as constants
  __device__ __forceinline__ float ox(int idx) const { return (float)c_pat[idx][0]; }
  __device__ __forceinline__ float oy(int idx) const { return (float)c_pat[idx][1]; }
  __device__ __forceinline__ float ref(float color) const { return 1.0f * color + 0.0f; }
};
struct TracePatOn {       // traceOn: Rplane * patternP (:628, :636-637) and hostToFrame_affine
  const float (&rot)[8][2];
  const float aff0, aff1;
  __device__ __forceinline__ float ox(int idx) const { return rot[idx][0]; }
  __device__ __forceinline__ float oy(int idx) const { return rot[idx][1]; }
  __device__ __forceinline__ float ref(float color) const { return aff0 * color + aff1; }
};

// ---- the energy of the search step at (ptx, pty).  No `#pragma unroll` on the tap loop: the helper is optimised on its own before it is
// inlined, and unrolled there it made k_trace_stereo_blk load and convert all of c_pat up front and keep it in 16 VGPRs (74 instead of 58:
// 6 waves per SIMD instead of 8).  The constant trip count unrolls it in the kernel, which the pattern reads with constant indices need.
template <class Pat>
__device__ __forceinline__ float trace_step_energy(const Pat& P, const float* plane, const int wG0, const float* color, const float ptx, const float pty) {
  float energy = 0;
  for (int idx = 0; idx < 8; idx++) {
    const float hitColor = interp31_plane(plane, (float)(ptx + P.ox(idx)), (float)(pty + P.oy(idx)), wG0);
    if (!isfinite(hitColor)) { energy += 1e5; continue; }
    const float residual = hitColor - (float)P.ref(color[idx]);
    const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
    energy += hw * residual * residual * (2 - hw);
  }
  return energy;
}

// ---- the first minimum over steps s = pass * 64 + lane < nsteps of one wave (the reference takes strictly smaller energies only, in step
// order: the earliest of equal steps wins) and the smallest energy outside bI +- kMinTraceTestRadius.  bI < 0: no step at all.
struct TraceMin { float bE, bX, bY, secondBest; int bI; };
__device__ __forceinline__ TraceMin trace_first_min(const int nsteps, const int lane, const float (&myE)[2], const float (&myX)[2], const float (&myY)[2]) {
  float bE = 1e10f; int bI = -1; float bX = 0, bY = 0;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int s = pass * 64 + lane;
    if (s < nsteps && myE[pass] < bE) { bE = myE[pass]; bI = s; bX = myX[pass]; bY = myY[pass]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oE = __shfl_xor(bE, o, 64); const int oI = __shfl_xor(bI, o, 64);
    const float oX = __shfl_xor(bX, o, 64), oY = __shfl_xor(bY, o, 64);
    const bool take = (oI >= 0) && (bI < 0 || oE < bE || (oE == bE && oI < bI));
    if (take) { bE = oE; bI = oI; bX = oX; bY = oY; }
  }
  float secondBest = 1e10f;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int s = pass * 64 + lane;
    if (s < nsteps && (s < bI - kMinTraceTestRadius || s > bI + kMinTraceTestRadius) && myE[pass] < secondBest) secondBest = myE[pass];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) secondBest = fminf(secondBest, __shfl_xor(secondBest, o, 64));
  return TraceMin{bE, bX, bY, secondBest, bI};
}

// ---- DSO-native sub-pixel Gauss-Newton (:707-769).  An iteration is: trace_gn_terms for each of the eight pattern pixels; the kernel's
// own sum in pattern order (H from 1; a non-finite sample adds 1e5 to the energy and nothing else); trace_gn_advance.
struct TraceGNTerms { float tH, tb, te; int nan; };
template <class Pat>
__device__ __forceinline__ TraceGNTerms trace_gn_terms(const Pat& P, const float patx, const float paty, const float4* __restrict__ dI, const int wG0, const float bestU,
                                                       const float bestV, const float dx, const float dy, const float col, const float wgt) {
  TraceGNTerms t = {0, 0, 0, 0};
  const float3 hit = interp33(dI, (float)(bestU + patx), (float)(bestV + paty), wG0);
  if (!isfinite(hit.x)) t.nan = 1;
  else {
    const float residual = hit.x - P.ref(col);
    const float dResdDist = dx * hit.y + dy * hit.z;
    const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
    t.tH = hw * dResdDist * dResdDist;
    t.tb = hw * residual * dResdDist;
    t.te = wgt * wgt * hw * residual * residual * (2 - hw);
  }
  return t;
}
struct TraceGN {
  float bestU, bestV, bestEnergy, uBak, vBak, stepBack;
  __device__ __forceinline__ TraceGN(float u, float v, float e) : bestU(u), bestV(v), bestEnergy(kTraceGNIterations > 0 ? 1e5f : e), uBak(u), vBak(v), stepBack(0) {}
};
// accepts the step of (H, bb) or goes half the last step back; true: the refinement stops here
__device__ __forceinline__ bool trace_gn_advance(TraceGN& S, const float H, const float bb, const float energy, const float dx, const float dy) {
  const float gnstepsize = 1;
  if (energy > S.bestEnergy) {
    S.stepBack *= 0.5;
    S.bestU = S.uBak + S.stepBack * dx;
    S.bestV = S.vBak + S.stepBack * dy;
  } else {
    float step = -gnstepsize * bb / H;
    if (step < -0.5) step = -0.5;
    else if (step > 0.5) step = 0.5;
    if (!isfinite(step)) step = 0;
    S.uBak = S.bestU;
    S.vBak = S.bestV;
    S.stepBack = step;
    S.bestU += step * dx;
    S.bestV += step * dy;
    S.bestEnergy = energy;
  }
  return fabsf(S.stepBack) < kTraceGNThreshold;
}

// ---- the idepth interval of (bestU, bestV) -+ errorInPixel along the line, in order
__device__ __forceinline__ void trace_interval(const float (&pr)[3], const float (&Kt)[3], const float bestU, const float bestV, const float dx, const float dy,
                                               const float errorInPixel, float& idepth_min_stereo, float& idepth_max_stereo) {
  if (dx * dx > dy * dy) {
    idepth_min_stereo = (pr[2] * (bestU - errorInPixel * dx) - pr[0]) / (Kt[0] - Kt[2] * (bestU - errorInPixel * dx));
    idepth_max_stereo = (pr[2] * (bestU + errorInPixel * dx) - pr[0]) / (Kt[0] - Kt[2] * (bestU + errorInPixel * dx));
  } else {
    idepth_min_stereo = (pr[2] * (bestV - errorInPixel * dy) - pr[1]) / (Kt[1] - Kt[2] * (bestV - errorInPixel * dy));
    idepth_max_stereo = (pr[2] * (bestV + errorInPixel * dy) - pr[1]) / (Kt[1] - Kt[2] * (bestV + errorInPixel * dy));
  }
  if (idepth_min_stereo > idepth_max_stereo) { const float t = idepth_min_stereo; idepth_min_stereo = idepth_max_stereo; idepth_max_stereo = t; }
}

}  // namespace sdso
