// Per-residual state of the BA window between linearisations (reference paths under its root):
//   k_ba_apply          PointFrameResidual::applyRes(true) + EFResidual::takeDataF   Residuals.cpp:367-385, EnergyFunctionalStructs.cpp:37-51
//   k_ba_post_state     linearizeAll_Reductor(fixLinearization = true) per residual  FullSystemOptimize.cpp:62-78; the projections of
//                       Residuals.cpp:130-131, :215-225
//   k_ba_fixlin         EFResidual::fixLinearizationF                                EnergyFunctionalStructs.cpp:96-123
//   k_ba_reset_flagged  resetOOB + isLinearized = false for flagged points           FullSystem.cpp:1012-1016
//   k_ba_unmask         ends k_ba_reset_flagged's temporary exclusion
//   k_ba_init_res       the state of a fresh PointFrameResidual                      Residuals.cpp:40-52
//   k_ba_reset_all      resetOOB for every non-linearized residual                   FullSystemOptimize.cpp:886-892
namespace sdso {

// ------------------------------------------------------------------ applyRes(true) + takeDataF
// one lane per residual that is not linearized (nor temporarily excluded: k_ba_reset_flagged)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_apply(const BaDev* __restrict__ wins, int cond = 0) {
  const BaDev& B = wins[blockIdx.y];
  if (ba_gate_skip(B, cond)) return;
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr) return;
  float* jp = B.r_rec + (size_t)B.r_orig[i] * 16;
  float* tm = jp + 8;
  if (B.r_lin[i]) return;
  const uint8_t st = B.r_state[i];
  if (st == 1) return;  // can never go back from OOB
  const uint8_t ns = B.r_newState[i];
  uint8_t act = 0;
  if (ns == 0) {
    act = 1;
    const uint8_t sel = B.r_jsel[i] ^ 1;
    B.r_jsel[i] = sel;
    float jl[76], out[8];   // (only the groups takeDataF reads are loaded)
#pragma unroll
    for (int k = 0; k < 6; k++) load_J_group(B.J[sel], B.nrp, i, kTakeDataGroups[k], jl);
    JAC_TAKE_DATA(out);
    *(float4*)(jp) = make_float4(out[0], out[1], out[2], out[3]);
    *(float4*)(jp + 4) = make_float4(out[4], out[5], out[6], out[7]);
  }
  else {
    // the records of a residual that is not active hold zeros (like the fused kernel's): the Schur kernel adds / multiplies records without
    // looking at their flags
    *(float4*)(jp) = make_float4(0.f, 0.f, 0.f, 0.f);
    *(float4*)(jp + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    *(float4*)(tm) = make_float4(0.f, 0.f, 0.f, 0.f);
    tm[4] = 0.f; tm[5] = 0.f;
  }
  B.r_act[i] = act;
  jp[RR_FLAGS] = (float)act;
  B.r_state[i] = ns;
  B.r_energy[i] = B.r_newEnergy[i];
}

// What FullSystem::linearizeAll_Reductor(fixLinearization = true) does per residual after applyRes (FullSystemOptimize.cpp:62-78) at the end
// of FullSystem::optimize, and the projections that closing linearisation left in the PointFrameResidual (centerProjectedTo, projectedTo:
// Residuals.cpp:130-131, :215-225 — LIN_PROJECT_FEJ / project_pattern of ba_lin.hip, re-evaluated here so that the hot kernels need not
// store them).
// One lane per residual; PointHessian::maxRelBaseline / numGoodResiduals through integer atomics (order-independent: non-negative floats
// compare like their bit patterns).  proj: nr x 19 (projectedTo 16, centerProjectedTo 3), zeros for residuals that are not active.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_post_state(const BaDev* __restrict__ wins, float* __restrict__ proj, int counters /* 0: the projections only */) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr) return;
  if (!proj && !counters) return;
  float scratch[19];
  float* pj = proj ? proj + (size_t)i * 19 : scratch;   // proj == nullptr: the counters only (the end of an optimize call)
#pragma unroll
  for (int k = 0; k < 19; k++) pj[k] = 0.f;
  if ((B.r_lin[i] & 1) || !B.r_act[i]) return;       // not in activeResiduals (:880-889) / on toRemove (:80-84)
  const int h = B.r_host[i], t = B.r_target[i], pt = B.r_point[i];
  const float* __restrict__ pre = B.t_precalc + (size_t)(h * B.nf + t) * 27;
  const float* KRKi = pre; const float* Kt = pre + 9; const float* R0 = pre + 12; const float* t0 = pre + 21;
  const float4 g = B.p_geo[pt];
  const float pu = g.x, pv = g.y, idepth_scaled = g.z, idepth_zero_scaled = g.w;
  {
    const float fxl = B.fxl, fyl = B.fyl, cxl = B.cxl, cyl = B.cyl, fxli = B.fxli, fyli = B.fyli;
    LIN_PROJECT_FEJ((void)0);   // (no exit: an active residual has passed them)
    pj[16] = Ku0; pj[17] = Kv0; pj[18] = new_idepth;
  }
  project_pattern<2>(KRKi, Kt, pu, pv, idepth_scaled, B.wM3, B.hM3, pj, pj + 1);
  if (!counters || !B.r_isnew[i]) return;
  float pinf[3], pp[3];                               // FullSystemOptimize.cpp:64-76
#pragma unroll
  for (int r = 0; r < 3; r++) { pinf[r] = (KRKi[r * 3 + 0] * pu + KRKi[r * 3 + 1] * pv) + KRKi[r * 3 + 2] * 1.0f; pp[r] = pinf[r] + Kt[r] * idepth_scaled; }
  const float dx = pinf[0] / pinf[2] - pp[0] / pp[2], dy = pinf[1] / pinf[2] - pp[1] / pp[2];
  const float relBS = (float)(0.01 * (double)sqrtf(dx * dx + dy * dy));
  int* tr = (int*)(B.p_track + pt);
  if (relBS == relBS) atomicMax(tr, __float_as_int(relBS));   // if (relBS > p->maxRelBaseline) p->maxRelBaseline = relBS
  atomicAdd(tr + 1, 1);                                       // p->numGoodResiduals++
}

// fixLinearizationF for the active residuals of flagged points; sets isLinearized
__global__ __launch_bounds__(BA_BLOCK) void k_ba_fixlin(const BaDev* __restrict__ wins, const uint8_t* __restrict__ pflag) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr) return;
  const int pt = B.r_point[i];
  if (!pflag[pt] || !B.r_act[i]) return;
  float jl[76];
  load_J(B.J[B.r_jsel[i]], B.nrp, i, jl);
  const int S = B.nrp;
  const float* dp = B.t_adHTdelta + (size_t)(B.r_host[i] + B.nf * B.r_target[i]) * 8;
  float dx, dy;
  jac_delta(jl, dp, B.t_cdelta, B.p_delta[pt], dx, dy);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    float rtz = JV(J_RESF + k);
    rtz = rtz - JV(J_IDX0 + k) * dx;
    rtz = rtz - JV(J_IDX1 + k) * dy;
    rtz = rtz - JV(J_AB0 + k) * dp[6];
    rtz = rtz - JV(J_AB1 + k) * dp[7];
    B.r_toZero[k * S + i] = rtz;
  }
  B.r_lin[i] = 1;
  B.r_rec[(size_t)B.r_orig[i] * 16 + RR_FLAGS] = 3.f;  // active | linearized
}

// PointFrameResidual::resetOOB (Residuals.h:106-112) of one residual
__device__ __forceinline__ void reset_oob(const BaDev& B, int i) { B.r_energy[i] = 0; B.r_newEnergy[i] = 0; B.r_newState[i] = 2; B.r_state[i] = 0; }
// resetOOB + isLinearized=false for the residuals of flagged points (FullSystem.cpp:1012-1016)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_reset_flagged(const BaDev* __restrict__ wins, const uint8_t* __restrict__ pflag) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr) return;
  if (!pflag[B.r_point[i]]) { B.r_lin[i] |= 2; return; }  // bit1: temporarily excluded from linearize/apply
  reset_oob(B, i);
  B.r_lin[i] = 0;
}
__global__ __launch_bounds__(BA_BLOCK) void k_ba_unmask(const BaDev* __restrict__ wins) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i < B.nr) B.r_lin[i] &= 1;
}
// upload: state_NewState = OUTLIER, state_NewEnergyWithOutlier = -1 (Residuals.cpp:40-52)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_init_res(const BaDev* __restrict__ wins) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr) return;
  B.r_newState[i] = 2;
  B.r_newEnergyWO[i] = -1.f;
}
// resetOOB for every non-linearized residual (FullSystemOptimize.cpp:886-892)
__global__ __launch_bounds__(BA_BLOCK) void k_ba_reset_all(const BaDev* __restrict__ wins) {
  const BaDev& B = wins[blockIdx.y];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= B.nr || B.r_lin[i]) return;
  reset_oob(B, i);
}

#undef LIN_PROJECT_FEJ

}  // namespace sdso
