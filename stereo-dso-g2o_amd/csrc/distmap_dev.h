// Device functions of the CoarseDistanceMap kernels that more than one translation unit needs: the projection into the level-1 map and
// the per-candidate gates of activatePointsMT STEP 2 (FullSystem.cpp:850-887).  k_select_classify (distmap.hip) applies them to arrays
// the caller uploaded, k_imm_act_classify (imm_activate.hip) to the blobs of the device-resident immature points.
#pragma once
#include "sdso_internal.h"

namespace sdso {

enum { DM_KEEP = 0, DM_DELETE = 1, DM_SELECT = 2, DM_PENDING = 3 };

// KRKi * (u, v, 1) + Kt * idepth in the unfused left-to-right order of Eigen's 3x3 product, then the rounding of
// CoarseTracker.cpp:1243-1246 / FullSystem.cpp:884-887.  A quotient that is not finite or does not fit an int is "outside".
__device__ __forceinline__ bool dm_project(const sdso_distmap_geom_t& g, float u, float v, float idepth, int w1, int h1, int& iu, int& iv, float& ptp0) {
  const float p0 = ((g.KRKi[0] * u + g.KRKi[1] * v) + g.KRKi[2] * 1.f) + g.Kt[0] * idepth;
  const float p1 = ((g.KRKi[3] * u + g.KRKi[4] * v) + g.KRKi[5] * 1.f) + g.Kt[1] * idepth;
  const float p2 = ((g.KRKi[6] * u + g.KRKi[7] * v) + g.KRKi[8] * 1.f) + g.Kt[2] * idepth;
  const float qx = p0 / p2 + 0.5f, qy = p1 / p2 + 0.5f;
  ptp0 = p0;
  if (!(qx > -2.0e9f && qx < 2.0e9f && qy > -2.0e9f && qy < 2.0e9f)) return false;
  iu = (int)qx;
  iv = (int)qy;
  return iu > 0 && iv > 0 && iu < w1 && iv < h1;
}

// The gates of one candidate that do not depend on the map.  `c` hands out the candidate's members on demand (status, imax, imin,
// interval, quality, flagged, geom, u, v), so a caller loads only what the taken branch reads.  DM_PENDING: the candidate goes on to the
// distance test at (iu, iv) with the fraction `frac` of :889.
template <class Cand>
__device__ __forceinline__ uint8_t dm_classify(const Cand& c, float minTraceQuality, int w1, int h1, int& iu, int& iv, float& frac) {
  const uint8_t st = c.status();
  const float imax = c.imax(), imin = c.imin();
  if (!isfinite(imax) || st == 2 /* IPS_OUTLIER */) return DM_DELETE;                  // :850-856
  const bool can = (st == 0 || st == 3 || st == 4 || st == 1) && c.interval() < 8 && c.quality() > minTraceQuality && (imax + imin) > 0;   // :860-866
  if (!can) return (c.flagged() || st == 1 /* IPS_OOB */) ? DM_DELETE : DM_KEEP;      // :869-880
  float p0;
  if (dm_project(c.geom(), c.u(), c.v(), 0.5f * (imax + imin), w1, h1, iu, iv, p0)) {  // :883-887
    frac = p0 - floorf(p0);                                                            // :889 — ptp[0], not the quotient
    return DM_PENDING;
  }
  return DM_DELETE;                                                                    // :897-900
}

// distmap.hip: the map of the ctx and the order-dependent rest of STEP 2 on device arrays (k_distmap_select, enqueue only)
bool distmap_dims(sdso_ctx* ctx, int* w1, int* h1);   // false: no map has been made yet
int dm_run_select(sdso_ctx* ctx, int n, uint8_t* dec, const int* iu, const int* iv, const float* frac, const float* thr, int mode_add, int* n_selected);

}  // namespace sdso
