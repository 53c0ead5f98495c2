// The BA linearisation: PointFrameResidual::linearize (src/FullSystem/Residuals.cpp:83-336 of the reference) per residual, in the
// reference's operation order — J, energies and states are bit-identical to the CPU path.
//   LIN_* / project_pattern  every statement of that arithmetic, ONCE, for all who evaluate it
//   linearize_one            one residual per lane with its own loads: k_ba_linearize (the un-fused path)
//   coop_gather_hits         the cooperative quad gather (CG_*, tap_rsrc_t) ...
//   linearize_coop           ... and the linearisation around it: k_ba_lin_fused (ba_top.hip)
//   k_ba_linearize           linearize for every residual that is not linearized, and the energy partials
// k_ba_post_state (ba_state.hip) re-evaluates LIN_PROJECT_FEJ / project_pattern for the projections the hot kernels do not store.
namespace sdso {

__constant__ int c_pattern[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};

// ------------------------------------------------------------------ the statements of linearize, once
// The pieces are macros, not force-inlined functions: k_ba_lin_fused's instruction stream (102 / 101 VGPRs, four workgroups per CU,
// tests/test_lin_isa_cpu.py) follows the ORDER in which the statements reach the compiler.  As functions over a struct of the sums the
// optimised IR is the same set of instructions in another order, and the listing moves with it (+-0..17 instructions, the same or one
// VGPR fewer: profiles/ba_kernels_split_ab.txt); as macros the two linearisations expand to what they were, token for token.  Only
// project_pattern is a function: that one leaves the listing as it is.
// A piece reads and writes the names of the function that expands it:
//   template parameters STORE, KEEP;  B;  i, S, J, jl, rs (LIN_SETQ);  R0, t0, pu, pv, idepth_zero_scaled, fxl, fyl, cxl, cyl, fxli,
//   fyli (LIN_PROJECT_FEJ, LIN_GEO_JACOBIANS);  hit, idx, color, weights, affLL0, affLL1, b0, jab1, oob (LIN_PIXEL);  th, ns_out (LIN_FINISH)

// STORE: write the RawResidualJacobian groups to HBM (PointFrameResidual::J);  KEEP 1: leave them in jl[76]
// (device layout, ba_jac.h) for the caller;  KEEP 2: leave only the geometric groups and the 2x2 blocks in jl and return the
// five per-pixel sums of AccumulatedTopHessianSSE::addPoint<0> (resApprox = resF: JI_r[2], Jab_r[2], rr; same
// k = 0..7 order as AccumulatedTopHessian.cpp:119-128) in rs[5] — 35 fewer live registers.
#define LIN_SETQ(g, a, b, c, d)                                                          \
  do {                                                                                   \
    const f32x4 _q = {a, b, c, d};                                                       \
    if (STORE) gst_nt((f32x4*)(J + j_off(S, i, g)), _q); /* streamed, not re-read this iteration */ \
    if (KEEP == 1 || (KEEP == 2 && ((g) < 6 || (g) > 15))) { jl[4 * (g)] = _q.x; jl[4 * (g) + 1] = _q.y; jl[4 * (g) + 2] = _q.z; jl[4 * (g) + 3] = _q.w; } \
  } while (0)

// projectPoint (ResidualProjections.h:64-96) at the FEJ point: declares KliP, drescale, new_idepth, u, v, Ku0, Kv0.  OOB_EXIT is the
// statement that leaves when the point lies behind the camera or its centre outside the image
#define LIN_PROJECT_FEJ(OOB_EXIT)                                                        \
  float KliP[3];                                                                         \
  KliP[0] = (pu + 0 - cxl) * fxli;                                                       \
  KliP[1] = (pv + 0 - cyl) * fyli;                                                       \
  KliP[2] = 1;                                                                           \
  float ptp[3];                                                                          \
  _Pragma("unroll")                                                                      \
  for (int r = 0; r < 3; r++) ptp[r] = ((R0[r * 3 + 0] * KliP[0] + R0[r * 3 + 1] * KliP[1]) + R0[r * 3 + 2] * KliP[2]) + t0[r] * idepth_zero_scaled; \
  const float drescale = 1.0f / ptp[2];                                                  \
  const float new_idepth = idepth_zero_scaled * drescale;                                \
  if (!(drescale > 0)) OOB_EXIT;                                                         \
  const float u = ptp[0] * drescale;                                                     \
  const float v = ptp[1] * drescale;                                                     \
  const float Ku0 = u * fxl + cxl;                                                       \
  const float Kv0 = v * fyl + cyl;                                                       \
  if (!(Ku0 > 1.1f && Kv0 > 1.1f && Ku0 < B.wM3 && Kv0 < B.hM3)) OOB_EXIT

// Pass 1 (no memory traffic): project the 8 pattern pixels (pixel idx to Kus / Kvs[STRIDE * idx]); the residual is OOB — the return
// value — as soon as one leaves the image (Residuals.cpp:215-225).  Doing this first removes the early exit from the sampling loop, so
// the 32 bilinear taps are independent loads the hardware can keep in flight together.
template <int STRIDE>
__device__ __forceinline__ bool project_pattern(const float* KRKi, const float* Kt, float pu, float pv, float idepth_scaled, float wM3, float hM3, float* Kus, float* Kvs) {
  bool oob = false;
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    const float up = pu + c_pattern[idx][0], vp = pv + c_pattern[idx][1];
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = ((KRKi[r * 3 + 0] * up + KRKi[r * 3 + 1] * vp) + KRKi[r * 3 + 2]) + Kt[r] * idepth_scaled;
    Kus[STRIDE * idx] = q[0] / q[2];
    Kvs[STRIDE * idx] = q[1] / q[2];
    if (!(Kus[STRIDE * idx] > 1.1f && Kvs[STRIDE * idx] > 1.1f && Kus[STRIDE * idx] < wM3 && Kvs[STRIDE * idx] < hM3)) oob = true;
  }
  return oob;
}

// Residuals.cpp:135-185: groups 0..5 from u, v, drescale, new_idepth, KliP
#define LIN_GEO_JACOBIANS()                                                              \
  {                                                                                      \
    float d_C_x[4], d_C_y[4];                                                            \
    const float d_d_x = drescale * (t0[0] - t0[2] * u) * SCALE_IDEPTH * fxl;             \
    const float d_d_y = drescale * (t0[1] - t0[2] * v) * SCALE_IDEPTH * fyl;             \
    d_C_x[2] = drescale * (R0[6] * u - R0[0]);                                           \
    d_C_x[3] = fxl * drescale * (R0[7] * u - R0[1]) * fyli;                              \
    d_C_x[0] = KliP[0] * d_C_x[2];                                                       \
    d_C_x[1] = KliP[1] * d_C_x[3];                                                       \
    d_C_y[2] = fyl * drescale * (R0[6] * v - R0[3]) * fxli;                              \
    d_C_y[3] = drescale * (R0[7] * v - R0[4]);                                           \
    d_C_y[0] = KliP[0] * d_C_y[2];                                                       \
    d_C_y[1] = KliP[1] * d_C_y[3];                                                       \
    d_C_x[0] = (d_C_x[0] + u) * SCALE_F;                                                 \
    d_C_x[1] *= SCALE_F;                                                                 \
    d_C_x[2] = (d_C_x[2] + 1) * SCALE_C;                                                 \
    d_C_x[3] *= SCALE_C;                                                                 \
    d_C_y[0] *= SCALE_F;                                                                 \
    d_C_y[1] = (d_C_y[1] + v) * SCALE_F;                                                 \
    d_C_y[2] *= SCALE_C;                                                                 \
    d_C_y[3] = (d_C_y[3] + 1) * SCALE_C;                                                 \
    LIN_SETQ(0, new_idepth * fxl, 0, -new_idepth * u * fxl, -u * v * fxl);       /* Jpdxi[0][0..3] */                  \
    LIN_SETQ(1, (1 + u * u) * fxl, -v * fxl, 0, new_idepth * fyl);                /* Jpdxi[0][4..5], Jpdxi[1][0..1] */ \
    LIN_SETQ(2, -new_idepth * v * fyl, -(1 + v * v) * fyl, u * v * fyl, u * fyl); /* Jpdxi[1][2..5] */                 \
    LIN_SETQ(3, d_C_x[0], d_C_x[1], d_C_x[2], d_C_x[3]);                                 \
    LIN_SETQ(4, d_C_y[0], d_C_y[1], d_C_y[2], d_C_y[3]);                                 \
    LIN_SETQ(5, d_d_x, d_d_y, 0.f, 0.f);                                                 \
  }

// the eleven running sums of the eight pattern pixels, and the energy
#define LIN_DECLARE_SUMS()                                                               \
  float JIdxJIdx_00 = 0, JIdxJIdx_11 = 0, JIdxJIdx_10 = 0;                               \
  float JabJIdx_00 = 0, JabJIdx_01 = 0, JabJIdx_10 = 0, JabJIdx_11 = 0;                  \
  float JabJab_00 = 0, JabJab_01 = 0, JabJab_11 = 0;                                     \
  float wJI2_sum = 0, energyLeft = 0

// One pattern pixel (Residuals.cpp:227-300): hit = {I, dx, dy} of getInterpolatedElement33 (a float3 the piece may change); group
// 6 + idx; with KEEP 2 its terms of rs[5].  A sample that is not finite makes the residual OOB.
// PIN (linearize_coop asks for it, linearize_one never had it): every sum is complete, in a register, before the next pattern pixel
// starts.  Without these the compiler packs the eight pixels' terms into v_pk_* pairs ACROSS the loop, which keeps all eight pixels'
// products alive to its end: 147 VGPRs instead of 102 (three workgroups per CU instead of four; scratch in the variant without the
// stores).  The sums and their order are the same either way (profiles/lin_waits_ab.txt has both forms side by side).
#define LIN_PIXEL(PIN)                                                                   \
  {                                                                                      \
    if (!isfinite(hit.x)) oob = true;                                                    \
    const float residual = hit.x - (affLL0 * color[idx] + affLL1);                       \
    const float drdA = (color[idx] - b0);                                                \
    float wgt = sqrtf(kOutlierTHSumComponent / (kOutlierTHSumComponent + (hit.y * hit.y + hit.z * hit.z))); \
    wgt = 0.5f * (wgt + weights[idx]);                                                   \
    float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);              \
    energyLeft += wgt * wgt * hw * residual * residual * (2 - hw);                       \
    if (hw < 1) hw = sqrtf(hw);                                                          \
    hw = hw * wgt;                                                                       \
    hit.y *= hw;                                                                         \
    hit.z *= hw;                                                                         \
    LIN_SETQ(6 + idx, residual * hw, hit.y, hit.z, B.affA_fixed ? 0.f : drdA * hw);   /* resF, JIdx[0], JIdx[1], JabF[0] */ \
    jab1[idx] = B.affB_fixed ? 0.f : hw;                                                 \
    if (KEEP == 2) {                                                                     \
      const float ra = residual * hw;                                                    \
      rs[0] += ra * hit.y; rs[1] += ra * hit.z;                                          \
      rs[2] += ra * (B.affA_fixed ? 0.f : drdA * hw); rs[3] += ra * jab1[idx];           \
      rs[4] += ra * ra;                                                                  \
    }                                                                                    \
    JIdxJIdx_00 += hit.y * hit.y;                                                        \
    JIdxJIdx_11 += hit.z * hit.z;                                                        \
    JIdxJIdx_10 += hit.y * hit.z;                                                        \
    JabJIdx_00 += drdA * hw * hit.y;                                                     \
    JabJIdx_01 += drdA * hw * hit.z;                                                     \
    JabJIdx_10 += hw * hit.y;                                                            \
    JabJIdx_11 += hw * hit.z;                                                            \
    JabJab_00 += drdA * drdA * hw * hw;                                                  \
    JabJab_01 += drdA * hw * hw;                                                         \
    JabJab_11 += hw * hw;                                                                \
    wJI2_sum += hw * hw * (hit.y * hit.y + hit.z * hit.z);                               \
    if (PIN) {                                                                           \
      asm volatile("" : "+v"(JIdxJIdx_00), "+v"(JIdxJIdx_11), "+v"(JIdxJIdx_10), "+v"(JabJIdx_00), "+v"(JabJIdx_01), "+v"(JabJIdx_10), "+v"(JabJIdx_11)); \
      asm volatile("" : "+v"(JabJab_00), "+v"(JabJab_01), "+v"(JabJab_11), "+v"(wJI2_sum), "+v"(energyLeft)); \
      if (KEEP == 2) asm volatile("" : "+v"(rs[0]), "+v"(rs[1]), "+v"(rs[2]), "+v"(rs[3]), "+v"(rs[4])); \
    }                                                                                    \
  }

// groups 14..18, then the IN / OUTLIER rule (Residuals.cpp:302-336): ns_out = state_NewState, energyLeft becomes state_NewEnergy.
// BETWEEN is the caller's statement that takes state_NewEnergyWithOutlier (energyLeft as the pixels left it)
#define LIN_FINISH(BETWEEN)                                                              \
  LIN_SETQ(14, jab1[0], jab1[1], jab1[2], jab1[3]);                                      \
  LIN_SETQ(15, jab1[4], jab1[5], jab1[6], jab1[7]);                                      \
  LIN_SETQ(16, JIdxJIdx_00, JIdxJIdx_10, JIdxJIdx_10, JIdxJIdx_11);                      \
  LIN_SETQ(17, JabJIdx_00, JabJIdx_01, JabJIdx_10, JabJIdx_11);                          \
  LIN_SETQ(18, JabJab_00, JabJab_01, JabJab_01, JabJab_11);                              \
  BETWEEN;                                                                               \
  if (energyLeft > th || wJI2_sum < 2) { energyLeft = th; ns_out = 2; }                  \
  else ns_out = 0

// ------------------------------------------------------------------ linearize, one residual per lane
// ns_out = state_NewState.  Returns the residual's term of the energy sum.
template <bool STORE, int KEEP>
__device__ __forceinline__ double linearize_one(const BaDev& B, int i, int h, int t, float* jl, int& ns_out, float* rs = nullptr) {
  B.r_newEnergyWO[i] = -1.f;
  ns_out = 1;
  const auto oob_exit = [&]() { B.r_newState[i] = 1; return (double)B.r_energy[i]; };
  if (B.r_state[i] == 1) return oob_exit();
  const int pt = B.r_point[i];
  const float* __restrict__ pre = B.t_precalc + (size_t)(h * B.nf + t) * 27;
  const float* KRKi = pre; const float* Kt = pre + 9; const float* R0 = pre + 12; const float* t0 = pre + 21;
  const float affLL0 = pre[24], affLL1 = pre[25], b0 = pre[26];
  const float4 g = B.p_geo[pt];
  const float pu = g.x, pv = g.y, idepth_scaled = g.z, idepth_zero_scaled = g.w;
  const char* __restrict__ dIl = B.t_img[t];
  float* __restrict__ J = STORE ? (B.r_jsel[i] != 0 ? B.J[0] : B.J[1]) : nullptr;   // PointFrameResidual::J: the slot EFResidual::J is not in
  const int S = B.nrp;
  const float fxl = B.fxl, fyl = B.fyl, cxl = B.cxl, cyl = B.cyl, fxli = B.fxli, fyli = B.fyli;

  LIN_PROJECT_FEJ(return oob_exit());
  if (B.r_proj) { float* pj = B.r_proj + (size_t)i * 19; pj[16] = Ku0; pj[17] = Kv0; pj[18] = new_idepth; }
  LIN_GEO_JACOBIANS();

  LIN_DECLARE_SUMS();
  const float4 c0 = *(const float4*)(B.p_color + (size_t)pt * 8), c1 = *(const float4*)(B.p_color + (size_t)pt * 8 + 4);
  const float4 w0 = *(const float4*)(B.p_weights + (size_t)pt * 8), w1 = *(const float4*)(B.p_weights + (size_t)pt * 8 + 4);
  const float color[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float weights[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  float Kus[8], Kvs[8];
  bool oob = project_pattern<1>(KRKi, Kt, pu, pv, idepth_scaled, B.wM3, B.hM3, Kus, Kvs);
  if (oob) return oob_exit();
  float jab1[8];
  // the taps are fetched in two groups of 4 pattern pixels (16 gathers in flight per lane): half the registers
  // of one group of 32
#pragma unroll
  for (int hb = 0; hb < 8; hb += 4) {
    float3 hits[4];
#pragma unroll
    for (int k = 0; k < 4; k++) hits[k] = interp33_tiled(dIl, Kus[hb + k], Kvs[hb + k], B.tiledT);
#pragma unroll
    for (int idx = hb; idx < hb + 4; idx++) {
      if (B.r_proj) { B.r_proj[(size_t)i * 19 + idx * 2] = Kus[idx]; B.r_proj[(size_t)i * 19 + idx * 2 + 1] = Kvs[idx]; }
      float3 hit = hits[idx - hb];
      LIN_PIXEL(false);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the second group's gathers behind the first group's arithmetic
  }
  if (oob) return oob_exit();
  const float th = fmaxf(B.t_frameTH[h], B.t_frameTH[t]);
  LIN_FINISH(B.r_newEnergyWO[i] = energyLeft);
  B.r_newState[i] = (uint8_t)ns_out;
  B.r_newEnergy[i] = energyLeft;
  return (double)energyLeft;
}

// ------------------------------------------------------------------ linearize, the taps of a wave fetched together
// The same linearisation for the fused kernel, with the 32 bilinear taps of every residual fetched COOPERATIVELY: the taps of one
// residual sit on 32 neighbouring lanes of ONE load instruction (pixel-major, the four corners of a pixel adjacent), so an
// instruction touches ~16 distinct 128-B lines instead of 64 and no line is asked for twice.  On gfx950 a divergent 16-byte load costs per distinct line, not
// per byte: with one residual per lane the 32 taps run at 105 G lane-taps/s whatever HBM could deliver (tools/mix_bw.hip);
// spread over lanes the same taps run at the HBM rate.  The interpolated samples travel through a wave-private LDS stage back
// to the residual's own lane, which then expands the same LIN_* pieces as linearize_one — every per-residual result stays
// bit-identical.  Must be called by ALL lanes of the wave
// (`live` = this lane has a residual to linearise); early exits of linearize_one become the `dead` flag.
// Stage of one wave: the 8 pattern-pixel coordinates of its 64 residuals (float2 each), and the interpolated {I, dx, dy}
// of every pattern pixel in rows of 65 floats ([pixel*3 + channel][residual]).
constexpr int CG_COORD_FLOATS = 64 * 8 * 2, CG_ROW = 64, CG_HIT_FLOATS = 8 * 3 * CG_ROW, CG_WAVE_FLOATS = CG_COORD_FLOATS + CG_HIT_FLOATS;
constexpr int CG_BATCH = 8;                                   // loads in flight per lane
// The target image as a raw buffer: 32-bit byte offsets from a base in SGPRs, and a range check that turns a load which must not happen into
// zeros.  The range is 2 GiB whatever the image's size (every offset a live lane forms lies inside the image), TAP_OFF_DEAD lies beyond it.
typedef __amdgpu_buffer_rsrc_t tap_rsrc_t;
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
constexpr unsigned TAP_RANGE = 0x80000000u, TAP_OFF_DEAD = 0xfffffff0u;   // (the window upload, ba_window.hip, refuses an image of TAP_RANGE bytes or more)
constexpr int TAP_RSRC_FLAGS = 0x00020000;   // word 3 of a gfx9 (gfx950) raw buffer descriptor: DATA_FORMAT = 32; other families lay this word out differently
// All 32 bilinear taps of a residual in ONE load instruction: round r serves residuals 2r and 2r+1 of the wave, lane = (residual,
// pattern pixel, corner).  The four corner lanes of a pixel exchange their samples inside the quad and evaluate
// getInterpolatedElement33 (same expression, same order: bit-identical to interp33); the corner-0 lane parks the result for the
// residual's own lane.  A residual's image lines are touched by exactly one instruction, so they are fetched once.
__device__ __forceinline__ void coop_gather_hits(tap_rsrc_t img /* wave-uniform: SGPRs */, int T, bool dead, const float* Ku, const float* Kv, float* wstage) {
  const int lane = threadIdx.x & 63;
  float2* coords = (float2*)wstage;
  float* hits = wstage + CG_COORD_FLOATS;
#pragma unroll
  for (int k = 0; k < 8; k++) coords[lane * 8 + k] = dead ? make_float2(-1.f, -1.f) : make_float2(Ku[k], Kv[k]);
  wave_lds_sync();
  const int sub = lane >> 5, px = (lane >> 2) & 7, c = lane & 3;
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += CG_BATCH) {
    // a batch: its eight coordinates out of LDS, its eight 12-byte tap loads back to back, ONE wait for the eight
    float qx[CG_BATCH], qy[CG_BATCH], qz[CG_BATCH];
    float2 cx[CG_BATCH];
#pragma unroll
    for (int r = 0; r < CG_BATCH; r++) cx[r] = coords[((r0 + r) * 2 + sub) * 8 + px];
#pragma unroll
    for (int r = 0; r < CG_BATCH; r++) {
      const int x = (int)cx[r].x + (c & 1), y = (int)cx[r].y + (c >> 1);
      // a dead residual's lanes ask for an offset beyond the descriptor's range: the hardware returns zeros and touches no memory (no branch
      // around the load, so no wait inside one)
      const u32x3 q = __builtin_amdgcn_raw_buffer_load_b96(img, cx[r].x >= 0 ? tile0_offset(x, y, T) : TAP_OFF_DEAD, 0, 0);
      qx[r] = __uint_as_float(q.x); qy[r] = __uint_as_float(q.y); qz[r] = __uint_as_float(q.z);
    }
    vm_wait_all();
#pragma unroll
    for (int r = 0; r < CG_BATCH; r++) {
      const int unit = (r0 + r) * 2 + sub;
      const float x = cx[r].x, y = cx[r].y;
      const int ix = (int)x;
      const int iy = (int)y;
      const float dx = x - ix;
      const float dy = y - iy;
      const float dxdy = dx * dy;
      // corners: lane c = 0 -> p00 (x, y), 1 -> p10 (x+1, y), 2 -> p01 (x, y+1), 3 -> p11.  Every corner lane scales its own
      // sample by its own weight; lane 0 adds the four products in the order of interp33: ((w11 p11 + w01 p01) + w10 p10) + w00 p00
      const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
      const float wa = (c & 1) ? w11 : w01, wb = (c & 1) ? w10 : w00;
      const float wc = (c & 2) ? wa : wb;
      const float tx = wc * qx[r], ty = wc * qy[r], tz = wc * qz[r];
      const float hx = ((quad_bcast<3>(tx) + quad_bcast<2>(tx)) + quad_bcast<1>(tx)) + tx;
      const float hy = ((quad_bcast<3>(ty) + quad_bcast<2>(ty)) + quad_bcast<1>(ty)) + ty;
      const float hz = ((quad_bcast<3>(tz) + quad_bcast<2>(tz)) + quad_bcast<1>(tz)) + tz;
      if (c == 0) {
        hits[(px * 3 + 0) * CG_ROW + unit] = hx;
        hits[(px * 3 + 1) * CG_ROW + unit] = hy;
        hits[(px * 3 + 2) * CG_ROW + unit] = hz;
      }
    }
  }
  wave_lds_sync();
}
// The fused kernel hands over what it has already fetched (k_ba_lin_fused: the pair's tables in SGPRs, the residual's scalars and the point's
// 80 bytes in one round trip each), so nothing is loaded here but the taps, and nothing this lane stores is read again: `fresh` = live and
// not sticky-OOB (state != 1); `energy_old` = r_energy[i].  Every lane state of linearize_one ends in ONE set of stores behind the
// Jacobian: r_newEnergyWO (-1 unless the residual was linearised to the end), r_newState, and r_newEnergy where it was.  Returns the
// residual's term of the energy sum (0 for a lane without a residual).
template <bool STORE, int KEEP>
__device__ __forceinline__ float linearize_coop(const BaDev& B, int i, bool live, bool fresh, const float* pre /* t_precalc of the pair */,
                                                tap_rsrc_t img, float th /* max of the two frames' thresholds */, f32x4 g, f32x4 c0, f32x4 c1,
                                                f32x4 w0, f32x4 w1, uint8_t jsel, float energy_old, float* jl, int& ns_out, float* rs, float* wstage) {
  ns_out = 1;
  bool dead = true;
  float Kus[8], Kvs[8], jab1[8];
  bool oob = false;
  float g_u = 0, g_v = 0, g_dr = 0, g_nid = 0, g_k0 = 0, g_k1 = 0;
  LIN_DECLARE_SUMS();
#pragma unroll
  for (int k = 0; k < 8; k++) { Kus[k] = 0; Kvs[k] = 0; jab1[k] = 0; }
  const float affLL0 = pre[24], affLL1 = pre[25], b0 = pre[26];
  const float color[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float weights[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const int S = B.nrp;
  float* const J = STORE ? ((jsel != 0) != (B.jfix != 0) ? B.J[0] : B.J[1]) : nullptr;   // jfix: EFResidual::J refreshed in place (ba_kernels.h)
  if (fresh) do {   // (the early exits of linearize_one leave `dead` set)
  const float* KRKi = pre; const float* Kt = pre + 9; const float* R0 = pre + 12; const float* t0 = pre + 21;
  const float pu = g.x, pv = g.y, idepth_scaled = g.z, idepth_zero_scaled = g.w;
  const float fxl = B.fxl, fyl = B.fyl, cxl = B.cxl, cyl = B.cyl, fxli = B.fxli, fyli = B.fyli;

  LIN_PROJECT_FEJ(break);
  g_u = u; g_v = v; g_dr = drescale; g_nid = new_idepth; g_k0 = KliP[0]; g_k1 = KliP[1];   // the geometric Jacobians are built after the taps (fewer live registers during the gathers)

  oob = project_pattern<1>(KRKi, Kt, pu, pv, idepth_scaled, B.wM3, B.hM3, Kus, Kvs);
  if (oob) break;
  dead = false;
  } while (0);
  coop_gather_hits(img, B.tiledT, dead, Kus, Kvs, wstage);
  if (!dead) {
  const float* hstage = wstage + CG_COORD_FLOATS + (threadIdx.x & 63);
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    float3 hit = make_float3(hstage[(idx * 3 + 0) * CG_ROW], hstage[(idx * 3 + 1) * CG_ROW], hstage[(idx * 3 + 2) * CG_ROW]);
    LIN_PIXEL(true);
  }
  }
  float ewo = -1.f, eret = live ? energy_old : 0.f;
  const bool done = !dead && !oob;
  if (done) {
  {
    const float* R0 = pre + 12; const float* t0 = pre + 21;
    const float u = g_u, v = g_v, drescale = g_dr, new_idepth = g_nid;
    const float KliP[2] = {g_k0, g_k1};
    const float fxl = B.fxl, fyl = B.fyl, fxli = B.fxli, fyli = B.fyli;
    LIN_GEO_JACOBIANS();
  }
  LIN_FINISH(ewo = energyLeft);
  eret = energyLeft;
  }
  if (live) {
    gst(B.r_newEnergyWO + i, ewo);
    gst(B.r_newState + i, (uint8_t)ns_out);
    if (done) gst(B.r_newEnergy + i, eret);
  }
  return eret;
}
#undef LIN_FINISH
#undef LIN_PIXEL
#undef LIN_DECLARE_SUMS
#undef LIN_GEO_JACOBIANS
#undef LIN_SETQ

__global__ __launch_bounds__(BA_BLOCK) void k_ba_linearize(const BaDev* __restrict__ wins, int cond = 0) {
  const BaDev& B = wins[blockIdx.y];
  if (ba_finished_lin(B) || ba_gate_skip(B, cond)) return;   // (a window whose resident loop has ended is left alone)
  if ((int)(blockIdx.x * BA_BLOCK) >= B.nr) return;
  __shared__ double lds[BA_BLOCK / 64];
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  double e = 0;
  int ns;
  if (i < B.nr && !B.r_lin[i]) e = linearize_one<true, 0>(B, i, B.r_host[i], B.r_target[i], nullptr, ns);
  e = block_sum_d(e, lds);
  if (threadIdx.x == 0) B.e_part[blockIdx.x] = e;
}

}  // namespace sdso
