// The kernels that run the epipolar search of trace_dev.h: k_immature_init (the constructor), k_trace_stereo_blk (traceStereo, a workgroup
// per 16 points) and trace_on_point / k_trace_on (traceOn, a wave per point).  The two searches differ only in lane layout and in where
// the geometry comes from.
__global__ __launch_bounds__(256) void k_immature_init(const float4* __restrict__ img, int w, int n, const float* __restrict__ u,
                                                       const float* __restrict__ v, float* __restrict__ color, float* __restrict__ weights,
                                                       float* __restrict__ gradH, float* __restrict__ energyTH) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float g0 = 0, g1 = 0, g2 = 0, g3 = 0;
  bool bad = false;
  for (int idx = 0; idx < 8; idx++) {
    const float3 ptc = interp33BiLin(img, u[p] + c_pat[idx][0], v[p] + c_pat[idx][1], w);
    color[p * 8 + idx] = ptc.x;
    if (!isfinite(ptc.x)) { bad = true; break; }
    g0 += ptc.y * ptc.y; g1 += ptc.y * ptc.z; g2 += ptc.z * ptc.y; g3 += ptc.z * ptc.z;
    weights[p * 8 + idx] = sqrtf(kOutlierTHSumComponent / (kOutlierTHSumComponent + (ptc.y * ptc.y + ptc.z * ptc.z)));
  }
  gradH[p * 4 + 0] = g0; gradH[p * 4 + 1] = g1; gradH[p * 4 + 2] = g2; gradH[p * 4 + 3] = g3;
  float e = 8 * kOutlierTH;
  e *= 1.0f * 1.0f;
  energyTH[p] = bad ? NAN : e;
}

// ImmaturePoint::traceStereo (ImmaturePoint.cpp:94-451), block organisation: a 256-thread workgroup owns PTS (16) points.
//   phase 1  thread t < PTS: the search line of point t, one LANE per point (the reference's scalar code; every early exit of
//                            ImmaturePoint.cpp:118-238 is a per-lane exit) -> numSteps, the steps' positions, direction in LDS
//   phase 2  wave w        : the discrete searches of its points, one after the other, lanes = steps
//   phase 3a lane (pt, px) : sub-pixel refinement, the 8 pattern pixels of a point on 8 neighbouring lanes
//   phase 3b thread t < PTS: quality, interval update, outputs
// The pieces are those of trace_dev.h, shared with trace_on_point below.
// (Rounds 1-3 ran one wave per point — every instruction of the geometry at 1 / 64 and of the refinement at 8 / 64 lanes, VALU-issue bound
// at 1 350 VALU instructions per point — and kept that kernel, an LDS-band variant of it and an 8-waves-per-SIMD build for A/B until
// round 5: 52-57 us against 33 us per 20 000 points, profiles/README.md.)  Same expressions, same operation order as the reference:
// bit-identical outputs.
// value of lane 8 (lane / 8) + K of a group of eight lanes (ds_swizzle_b32, bit mode: and 0x18, or K, inside each half of the wave)
template <int K>
__device__ __forceinline__ float tr_bcast8(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x18 | (K << 5))); }
template <int K>
__device__ __forceinline__ int tr_bcast8(int v) { return __builtin_amdgcn_ds_swizzle(v, 0x18 | (K << 5)); }
template <int K>
__device__ __forceinline__ double tr_bcast8(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)u, 0x18 | (K << 5)), hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(u >> 32), 0x18 | (K << 5));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
template <int GN_MODE, int PTS>   // PTS points per 256-thread workgroup (PTS / 4 searches per wave)
__global__ __launch_bounds__(256) void k_trace_stereo_blk(TraceDev T) {
  __shared__ int s_steps[PTS];                                   // 0: the point does not reach the search
  __shared__ float s_bE[PTS], s_bX[PTS], s_bY[PTS], s_second[PTS];
  __shared__ int s_bI[PTS];
  __shared__ float s_dx[PTS], s_dy[PTS], s_rU[PTS], s_rV[PTS], s_rE[PTS];   // search direction; the refined position and energy (phase 3a -> 3b)
  // the sample positions of every step of every point: ptx is the reference's running sum (ptx += dx, one rounding per step), so step s needs
  // s dependent additions — run by the point's OWN lane in phase 1 (64 points per instruction) instead of by every step lane of phase 2
  // (where the 45-trip loop was 40 % of a search's instructions).  Row stride 101: the 16..64 point lanes write distinct banks.
  constexpr int kStepCap = 100, kStepLd = kStepCap + 1;
  __shared__ float s_px[PTS * kStepLd], s_py[PTS * kStepLd];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int i = blockIdx.x * PTS + t;
  const float4* __restrict__ dI = T.img;
  const int wG0 = T.w, hG0 = T.h;
  const TracePatStereo pat;
  bool live = false;                                            // the point goes on to the search and the refinement
  // per-lane state that survives the barriers (thread t of phase 1 is thread t of phase 3)
  float u_stereo = 0, energyTH = 0, quality = 0, bf = 0;
  float Kt[3] = {0, 0, 0}, pr[3] = {0, 0, 0};
  TraceLine L = {};
  uint8_t prevStatus = 0;
  auto finish = [&](int st, float uvx, float uvy, float interval, bool writeUV) {
    T.lastTraceStatus[i] = (uint8_t)st;
    if (T.status) T.status[i] = (uint8_t)st;
    if (writeUV) { T.lastTraceUV[i * 2] = uvx; T.lastTraceUV[i * 2 + 1] = uvy; T.lastTracePixelInterval[i] = interval; }
    T.quality[i] = quality;
  };
  if (t < PTS) {
    s_steps[t] = 0;
    if (i < T.n) {
      if (T.skip && T.skip[i]) { if (T.status) T.status[i] = 255; }
      else {
        u_stereo = T.u_stereo[i];
        const float v_stereo = T.v_stereo[i];
        energyTH = T.energyTH[i];
        quality = T.quality[i];
        prevStatus = T.lastTraceStatus[i];
        const float bl0 = T.mode_right ? -T.baseline : T.baseline;
        Kt[0] = (T.fx * bl0 + 0.0f * 0.0f) + T.cx * 0.0f;
        Kt[1] = (0.0f * bl0 + T.fy * 0.0f) + T.cy * 0.0f;
        Kt[2] = (0.0f * bl0 + 0.0f * 0.0f) + 1.0f * 0.0f;
        bf = -T.fx * bl0;
        pr[0] = (1.0f * u_stereo + 0.0f * v_stereo) + 0.0f * 1.0f;
        pr[1] = (0.0f * u_stereo + 1.0f * v_stereo) + 0.0f * 1.0f;
        pr[2] = (0.0f * u_stereo + 0.0f * v_stereo) + 1.0f * 1.0f;
        const int st = trace_line(pr, Kt, T.idepth_min[i], T.idepth_min_stereo[i], T.idepth_max_stereo[i], T.gradH + (size_t)i * 4, wG0, hG0, L);
        if (st == IPS_OOB) finish(IPS_OOB, -1, -1, 0, true);
        else if (st != kTraceSearch) finish(st, 0, 0, 0, false);   // SKIPPED, BADCONDITION: lastTraceUV stays
        else {
          s_steps[t] = L.numSteps > 0 ? L.numSteps : 0;
          s_dx[t] = L.dx; s_dy[t] = L.dy;
          float px = L.ptx0, py = L.pty0;
          for (int k = 0; k < L.numSteps; k++) { s_px[t * kStepLd + k] = px; s_py[t * kStepLd + k] = py; px += L.dx; py += L.dy; }
          live = true;
        }
      }
    }
  }
  __syncthreads();

  // ---- phase 2: discrete search, one wave per point, lane = step
  // (unrolled over the wave's points, no branch around a point that does not search — its lanes are simply inactive — so that the
  // taps of the next point are in flight while the minimum of the current one is reduced)
#pragma unroll
  for (int pp = 0; pp < PTS / 4; pp++) {
    const int pt = wv * (PTS / 4) + pp;
    const int nsteps = s_steps[pt];
    const float* color = T.color + (size_t)(blockIdx.x * PTS + pt) * 8;
    float myE[2] = {1e30f, 1e30f}, myX[2] = {0, 0}, myY[2] = {0, 0};
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const int s = pass * 64 + lane;
      if (s < nsteps) {
        const float ptx = s_px[pt * kStepLd + s], pty = s_py[pt * kStepLd + s];
        myE[pass] = trace_step_energy(pat, T.plane, wG0, color, ptx, pty); myX[pass] = ptx; myY[pass] = pty;
      }
    }
    const TraceMin m = trace_first_min(nsteps, lane, myE, myX, myY);
    if (lane == 0 && nsteps > 0) { s_bE[pt] = m.bE; s_bI[pt] = m.bI; s_bX[pt] = m.bX; s_bY[pt] = m.bY; s_second[pt] = m.secondBest; }
  }
  __syncthreads();

  // ---- phase 3a: sub-pixel refinement, lane = (point, pattern pixel): the 8 samples of a pass are taken by 8 lanes at once and added in
  // pattern order on every lane of the group (the reference's sums, term by term); one lane per point walked them one after the other
  // (840 instructions and 6 dependent round trips per 16 points, with the other three waves of the workgroup idle)
#define TR_ALL8(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7)
  for (int q = t; q < PTS * 8; q += 256) {
    const int pl = q >> 3, idx = q & 7;
    if (s_steps[pl] <= 0) continue;                             // (all eight lanes of a point alike)
    const size_t gi = (size_t)blockIdx.x * PTS + pl;
    const float col = T.color[gi * 8 + idx], wgt = T.weights[gi * 8 + idx];
    const float dx = s_dx[pl], dy = s_dy[pl];
    float bestU = s_bX[pl], bestV = s_bY[pl], bestEnergy = s_bE[pl];
    if (s_bI[pl] < 0) { bestU = 0; bestV = 0; bestEnergy = 1e10f; }
    const float patx = pat.ox(idx), paty = pat.oy(idx);
    if constexpr (GN_MODE == 1) {
      // fork-live refinement (ImmaturePoint.cpp:309-412): VertexUVDSO in double, 8 EdgeTracePointUVDSO (dso_g2o_edge.cpp:571-619) with
      // Huber(9), one undamped g2o Gauss-Newton step per pass, update clamped by VertexUVDSO::oplusImpl (dso_g2o_vertex.cpp:73-88)
      double U = bestU, V = bestV;
      const double ddx = dx, ddy = dy;
      if (kTraceGNIterations > 0) bestEnergy = 1e5;
      for (int it = 0; it < kTraceGNIterations; it++) {
        double e = 0, J = 0;
        const bool inside = !((U - 2) < 0 || (U + 3) > (wG0 - 3) || (V - 2) < 0 || (V + 3) > (hG0 - 3));
        const float3 hit = interp33(dI, inside ? (float)(U + patx) : 2.5f, inside ? (float)(V + paty) : 2.5f, wG0);   // (outside: pixel (2,2), ignored)
        if (inside && isfinite(hit.x)) {
          e = hit.x - (1.0f * (double)col + 0.0f);
          J = ddx * hit.y + ddy * hit.z;
        }
        const float residual = e;
        const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
        const float te = wgt * wgt * hw * residual * residual * (2 - hw);
        const double e2 = e * e;
        const double rho1 = e2 <= (double)kHuberTH * kHuberTH ? 1. : kHuberTH / sqrt(e2);
        const double tb = rho1 * J * e, tH = J * rho1 * J;
        float energy = 0;
        double Hs = 0, bs = 0;
#define TR_ADD(K) energy += tr_bcast8<K>(te); bs -= tr_bcast8<K>(tb); Hs += tr_bcast8<K>(tH);
        TR_ALL8(TR_ADD)
#undef TR_ADD
        if (Hs != 0) {
          double update = bs / Hs;
          if (update < -0.5) update = -0.5;
          else if (update > 0.5) update = 0.5;
          else if (!isfinite(update)) update = 0;
          U += update * ddx;
          V += update * ddy;
        }
        if (!(energy > bestEnergy)) bestEnergy = energy;
      }
      bestU = U;
      bestV = V;
    } else {
      TraceGN S(bestU, bestV, bestEnergy);
      for (int it = 0; it < kTraceGNIterations; it++) {
        const TraceGNTerms g = trace_gn_terms(pat, patx, paty, dI, wG0, S.bestU, S.bestV, dx, dy, col, wgt);
        float H = 1, bb = 0, energy = 0;
#define TR_ADD(K) { const float h_ = tr_bcast8<K>(g.tH), b_ = tr_bcast8<K>(g.tb), e_ = tr_bcast8<K>(g.te); const int nn = tr_bcast8<K>(g.nan); \
                    if (nn) energy += 1e5; else { H += h_; bb += b_; energy += e_; } }
        TR_ALL8(TR_ADD)
#undef TR_ADD
        if (trace_gn_advance(S, H, bb, energy, dx, dy)) break;
      }
      bestU = S.bestU; bestV = S.bestV; bestEnergy = S.bestEnergy;
    }
    if (idx == 0) { s_rU[pl] = bestU; s_rV[pl] = bestV; s_rE[pl] = bestEnergy; }
  }
#undef TR_ALL8
  __syncthreads();

  // ---- phase 3b: outputs, one lane per point
  if (!live) return;
  {
    float bestEnergy0 = s_bE[t];
    if (s_bI[t] < 0) bestEnergy0 = 1e10f;
    const float newQuality = s_second[t] / bestEnergy0;
    if (newQuality < quality || L.numSteps > 10) quality = newQuality;
  }
  const float bestU = s_rU[t], bestV = s_rV[t], bestEnergy = s_rE[t];

  if (!(bestEnergy < energyTH * kTraceExtraSlack)) {
    finish(prevStatus == IPS_OUTLIER ? IPS_OOB : IPS_OUTLIER, -1, -1, 0, true);
    return;
  }
  float idepth_min_stereo, idepth_max_stereo;
  trace_interval(pr, Kt, bestU, bestV, L.dx, L.dy, L.errorInPixel, idepth_min_stereo, idepth_max_stereo);
  T.idepth_min_stereo[i] = idepth_min_stereo; T.idepth_max_stereo[i] = idepth_max_stereo;
  if (!isfinite(idepth_min_stereo) || !isfinite(idepth_max_stereo) || (idepth_max_stereo < 0)) { finish(IPS_OUTLIER, -1, -1, 0, true); return; }
  T.idepth_stereo[i] = (u_stereo - bestU) / bf;
  finish(IPS_GOOD, bestU, bestV, 2 * L.errorInPixel, true);
}

// ImmaturePoint::traceOn (ImmaturePoint.cpp:459-828): the same search along a general epipolar line, the same pieces on one wave per
// point: the line redundantly on every lane, lane = step in the search, pattern pixel idx on lane idx in the refinement.
// geom[pgeom[i]] is the hostToFrame geometry of the point's host; T.idepth_min_stereo / idepth_max_stereo hold idepth_min / idepth_max.
// trace_on_point is the body for point i of T on the calling wave; getG() yields the point's geometry (read only once the point is
// known to be traced).  k_trace_on runs it on uploaded arrays, k_imm_trace_on (imm_trace.hip) on the resident set.
template <class GetG>
__device__ __forceinline__ void trace_on_point(const TraceDev& T, const int i, GetG getG) {
  const int lane = threadIdx.x & 63;
  if (T.skip && T.skip[i]) { if (lane == 0 && T.status) T.status[i] = 255; return; }
  const float4* __restrict__ dI = T.img;
  const int wG0 = T.w, hG0 = T.h;
  const float u_stereo = T.u_stereo[i], v_stereo = T.v_stereo[i];
  float idepth_min_stereo = T.idepth_min_stereo[i], idepth_max_stereo = T.idepth_max_stereo[i];
  const float* color = T.color + (size_t)i * 8;
  const float* weights = T.weights + (size_t)i * 8;
  const float energyTH = T.energyTH[i];
  float quality = T.quality[i];
  const uint8_t prevStatus = T.lastTraceStatus[i];
  if (prevStatus == IPS_OOB) { if (lane == 0 && T.status) T.status[i] = IPS_OOB; return; }   // :466-468
  const sdso_trace_geom_t G = getG();

  auto finish = [&](int st, float uvx, float uvy, float interval, bool writeUV) {
    if (lane == 0) {
      T.lastTraceStatus[i] = (uint8_t)st;
      if (T.status) T.status[i] = (uint8_t)st;
      if (writeUV) { T.lastTraceUV[i * 2] = uvx; T.lastTraceUV[i * 2 + 1] = uvy; T.lastTracePixelInterval[i] = interval; }
      T.quality[i] = quality;
    }
  };

  const float Kt[3] = {G.Kt[0], G.Kt[1], G.Kt[2]};
  float pr[3];
#pragma unroll
  for (int r = 0; r < 3; r++) pr[r] = (G.KRKi[r * 3 + 0] * u_stereo + G.KRKi[r * 3 + 1] * v_stereo) + G.KRKi[r * 3 + 2] * 1.0f;
  float rot[8][2];
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    rot[idx][0] = G.KRKi[0] * (float)c_pat[idx][0] + G.KRKi[1] * (float)c_pat[idx][1];
    rot[idx][1] = G.KRKi[3] * (float)c_pat[idx][0] + G.KRKi[4] * (float)c_pat[idx][1];
  }
  const TracePatOn pat{rot, G.aff[0], G.aff[1]};
  TraceLine L;
  const int st = trace_line(pr, Kt, idepth_min_stereo, idepth_min_stereo, idepth_max_stereo, T.gradH + (size_t)i * 4, wG0, hG0, L);
  if (st == IPS_OOB) { finish(IPS_OOB, -1, -1, 0, true); return; }
  if (st != kTraceSearch) { finish(st, (L.uMax + L.uMin) * 0.5f, (L.vMax + L.vMin) * 0.5f, L.dist, true); return; }   // SKIPPED :525-531, BADCONDITION :596-603
  const float dx = L.dx, dy = L.dy;

  // ---- discrete search: lane = step (ptx is the reference's running sum ptx += dx)
  float myE[2] = {1e30f, 1e30f}, myX[2] = {0, 0}, myY[2] = {0, 0};
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int s = pass * 64 + lane;
    if (s < L.numSteps) {
      float ptx = L.ptx0, pty = L.pty0;
      for (int k = 0; k < s; k++) { ptx += dx; pty += dy; }
      myE[pass] = trace_step_energy(pat, T.plane, wG0, color, ptx, pty); myX[pass] = ptx; myY[pass] = pty;
    }
  }
  const TraceMin m = trace_first_min(L.numSteps, lane, myE, myX, myY);
  float bestU = m.bX, bestV = m.bY, bestEnergy = m.bE;
  if (m.bI < 0) { bestU = 0; bestV = 0; bestEnergy = 1e10f; }
  const float newQuality = m.secondBest / bestEnergy;
  if (newQuality < quality || L.numSteps > 10) quality = newQuality;

  // ---- sub-pixel refinement: pattern pixel idx on lane idx, summed in order
  const float patx = pat.ox(lane & 7), paty = pat.oy(lane & 7);   // (once: the 16-way select of a lane's row of rot)
  TraceGN S(bestU, bestV, bestEnergy);
  for (int it = 0; it < kTraceGNIterations; it++) {
    TraceGNTerms g = {0, 0, 0, 0};
    if (lane < 8) g = trace_gn_terms(pat, patx, paty, dI, wG0, S.bestU, S.bestV, dx, dy, color[lane], weights[lane]);
    float H = 1, bb = 0, energy = 0;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
      const float h_ = lane_bcast(g.tH, idx), b_ = lane_bcast(g.tb, idx), e_ = lane_bcast(g.te, idx);
      const int nn = lane_bcast(g.nan, idx);
      if (nn) { energy += 1e5; continue; }
      H += h_; bb += b_; energy += e_;
    }
    if (trace_gn_advance(S, H, bb, energy, dx, dy)) break;
  }

  if (!(S.bestEnergy < energyTH * kTraceExtraSlack)) {
    finish(prevStatus == IPS_OUTLIER ? IPS_OOB : IPS_OUTLIER, -1, -1, 0, true);
    return;
  }
  trace_interval(pr, Kt, S.bestU, S.bestV, dx, dy, L.errorInPixel, idepth_min_stereo, idepth_max_stereo);
  if (lane == 0) { T.idepth_min_stereo[i] = idepth_min_stereo; T.idepth_max_stereo[i] = idepth_max_stereo; }
  if (!isfinite(idepth_min_stereo) || !isfinite(idepth_max_stereo) || (idepth_max_stereo < 0)) { finish(IPS_OUTLIER, -1, -1, 0, true); return; }
  finish(IPS_GOOD, S.bestU, S.bestV, 2 * L.errorInPixel, true);
}
__global__ __launch_bounds__(256) void k_trace_on(TraceDev T, const sdso_trace_geom_t* __restrict__ geom, const int* __restrict__ pgeom) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= T.n) return;
  trace_on_point(T, i, [&] { return geom[pgeom[i]]; });
}
