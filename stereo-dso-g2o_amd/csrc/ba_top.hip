// The top of the BA system from the residuals (reference paths under its root):
//   TOP_OPERANDS_*   what one residual brings to AccumulatedTopHessianSSE::addPoint<mode>, once    AccumulatedTopHessian.cpp:36-198
//   top_emit         the operands' sums over a chunk on the matrix cores, in f64 -> top_part[chunk]
//   k_ba_accum_top   addPoint<mode> from the stored Jacobians: mode 0 active, 1 linearized, 2 marginalise
//   k_ba_lin_fused   the hot kernel: linearize (linearize_coop, ba_lin.hip) + applyRes(true) + takeDataF + addPoint<0> while the Jacobian
//                    is in registers                                                                Residuals.cpp:83-336, :367-385
//   k_ba_lenergy     EnergyFunctional::calcLEnergyPt                                                EnergyFunctional.cpp:354-417
//   k_ba_fold_top, k_ba_zero_topL   the chunks' partials of a pair -> the packed accumulator (stitchDoubleInternal reads it, ba_solve.hip)
namespace sdso {

// ------------------------------------------------------------------ top accumulation
// Block reduction of the 55 + 30 + 6 AccumulatorApprox sums (+ residual count) of one chunk -> top_part[chunk].
//
// The sums over the residuals of a chunk are  D = sum_i  u0_i (x) v0_i + u1_i (x) v1_i  with
//   u0 = [Jpdc0|Jpdxi0] (10), u1 = [Jpdc1|Jpdxi1] (10),
//   v0 = [a*u0 + b*u1 (10) | JabJIdx col 0 (2), JI_r0 | Jab2_00, Jab2_01, Jab_r0],
//   v1 = [b*u0 + c*u1 (10) | JabJIdx col 1 (2), JI_r1 | Jab2_11, Jab_r1, rr],
// plus a constant-1 row per half that turns the last three columns into plain sums: a 12 x 16 x (2*64) product
// per wave.  Summing 92 values over 64 lanes with shuffles costs ~1100 issue slots per residual; instead every
// lane parks its 26 values per half in a wave-private LDS panel (row stride 68 floats: conflict-free for the
// lane-contiguous writes and for the (row = lane%16, k = lane/16) reads) and the matrix cores do the reduction.
//
// The CROSS-RESIDUAL sums run in f64 (round 6): 2 x 16 v_mfma_f64_16x16x4_f64 per wave on the float operands converted exactly, two
// interleaved accumulators, the waves' tiles added in f64, top_part in f64, ONE rounding to float when the pair's chunks have been
// folded into the packed block.  The reference limits the growth of these float sums with its three-tier carry (MatrixAccumulators.h:
// 872-903) and its thread partials (AccumulatedTopHessian.cpp:299-308); a 128-term fmaf chain per wave (rounds 1-5) sat as far from an
// order-independent sum as the CPU path does but not on the same side, and north_star's 1e-5 on the pose update is at that distance
// (profiles/r05_truth_updates.txt).  In f64 the device's sums ARE the order-independent value up to one float rounding; what is left
// between device and CPU is the CPU float path's own distance from it (profiles/r06_truth_updates.txt).  The per-residual operands
// (v0 / v1 included) stay the float expressions they were: their roundings do not accumulate.
constexpr int TE_STRIDE = 68;
constexpr int TE_ROWS = 26;
constexpr int TE_WAVE_FLOATS = TE_ROWS * TE_STRIDE;
constexpr int TE_LDS_FLOATS = (BA_BLOCK / 64) * TE_WAVE_FLOATS;
typedef double te_d4 __attribute__((ext_vector_type(4)));
// Why f64 MFMA for the cross-residual / cross-point sums (measured on the 24 windows of tests/diag/truth_spread.py and the 256-window step,
// profiles/r06_acc_modes.txt): first pose update 1.4e-6 (median) from the f64-accumulator truth, the CPU float path 1.3e-5; +8 us on
// k_ba_lin_fused, +10 us on k_ba_sc_host per 256-window step (the f64 form runs at half the fp32 rate).  fp32 MFMA over 16-term chains added
// in f64 was free in time but only half way (6.4e-6: a chain's error grows with its partial sums, not with its length alone); one fp32 chain
// per wave (rounds 1-5) 1.1e-5.
static_assert(TE_LDS_FLOATS * 4 >= ((BA_BLOCK / 64) * 256 + BA_BLOCK / 64) * 8, "the waves' f64 tiles lie over the panels");

// What one residual brings to addPoint<mode> (AccumulatedTopHessian.cpp:100-172), as locals of the kernel that expands these (macros for
// the reason given in ba_lin.hip: k_ba_lin_fused's listing): x / y = [Jpdc | Jpdxi] rows 0 / 1, a b c = JIdx2, TR.. = JabJIdx and JI_r,
// br = Jab2, Jab_r, rr — zeros for a lane without an active residual — and TOP_OPERANDS_EMIT hands them to top_emit.
#define TOP_OPERANDS_DECLARE()                                                           \
  float x[10], y[10], a = 0, b = 0, c = 0;                                               \
  float TR00 = 0, TR10 = 0, TR01 = 0, TR11 = 0, TR02 = 0, TR12 = 0;                      \
  float br[6] = {0, 0, 0, 0, 0, 0};                                                      \
  _Pragma("unroll")                                                                      \
  for (int k = 0; k < 10; k++) { x[k] = 0; y[k] = 0; }
// jl: the residual's record (groups 0..5 and 16..18 suffice); JI_r0 .. rr: the five sums over the pattern of resApprox with JIdx[0], JIdx[1],
// JabF[0], JabF[1] and itself (:119-128).  BD, HDD, HCD[4]: where the residual's terms of the point's bd / Hdd / Hcd go (:160-172, the record)
#define TOP_OPERANDS_FILL(JI_r0, JI_r1, Jab_r0, Jab_r1, rr, BD, HDD, HCD)                \
  {                                                                                      \
    _Pragma("unroll")                                                                    \
    for (int k = 0; k < 4; k++) { x[k] = JV(J_C0 + k); y[k] = JV(J_C1 + k); }            \
    _Pragma("unroll")                                                                    \
    for (int k = 0; k < 6; k++) { x[4 + k] = JV(J_XI0 + k); y[4 + k] = JV(J_XI1 + k); }  \
    a = JV(J_IDX2 + 0); b = JV(J_IDX2 + 1); c = JV(J_IDX2 + 3);                          \
    TR00 = JV(J_ABIDX + 0); TR10 = JV(J_ABIDX + 1); TR01 = JV(J_ABIDX + 2); TR11 = JV(J_ABIDX + 3); \
    TR02 = JI_r0; TR12 = JI_r1;                                                          \
    br[0] = JV(J_AB2 + 0); br[1] = JV(J_AB2 + 1); br[2] = Jab_r0; br[3] = JV(J_AB2 + 3); br[4] = Jab_r1; br[5] = rr; \
    const float jdd0 = JV(J_DD + 0), jdd1 = JV(J_DD + 1);                                \
    const float q0 = a * jdd0 + b * jdd1;                                                \
    const float q1 = JV(J_IDX2 + 2) * jdd0 + c * jdd1;                                   \
    BD = JI_r0 * jdd0 + JI_r1 * jdd1;                                                    \
    HDD = q0 * jdd0 + q1 * jdd1;                                                         \
    _Pragma("unroll")                                                                    \
    for (int k = 0; k < 4; k++) HCD[k] = x[k] * q0 + y[k] * q1;                          \
  }
#define TOP_OPERANDS_EMIT(on, stage, chunk) top_emit(B, x, y, a, b, c, TR00, TR10, TR01, TR11, TR02, TR12, br, on, stage, chunk)

__device__ __forceinline__ void top_emit(const BaDev& B, const float* x, const float* y, float a, float b, float c, float TR00, float TR10, float TR01,
                                         float TR11, float TR02, float TR12, const float* br, bool on, float* stage, int chunk) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* S = stage + wv * TE_WAVE_FLOATS;
  const int m = lane & 15, kq = lane >> 4;
  const int mu = m < 10 ? m : 9;
  te_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};   // D[i][j], i = lane/16 + 4 v
  const unsigned long long onmask = __ballot(on);
#pragma unroll
  for (int ph = 0; ph < 2; ph++) {
    const float* u = ph ? y : x;
#pragma unroll
    for (int r = 0; r < 10; r++) S[r * TE_STRIDE + lane] = u[r];
#pragma unroll
    for (int cc = 0; cc < 10; cc++) S[(10 + cc) * TE_STRIDE + lane] = ph ? (b * x[cc] + c * y[cc]) : (a * x[cc] + b * y[cc]);
    S[20 * TE_STRIDE + lane] = ph ? TR10 : TR00;
    S[21 * TE_STRIDE + lane] = ph ? TR11 : TR01;
    S[22 * TE_STRIDE + lane] = ph ? TR12 : TR02;
#pragma unroll
    for (int q = 0; q < 3; q++) S[(23 + q) * TE_STRIDE + lane] = br[3 * ph + q];
    __syncthreads();
    const float one = (m == 10 + ph) ? 1.f : 0.f;
#pragma unroll
    for (int s4 = 0; s4 < 16; s4 += 2) {
      float av0 = S[mu * TE_STRIDE + 4 * s4 + kq], av1 = S[mu * TE_STRIDE + 4 * s4 + 4 + kq];
      av0 = m < 10 ? av0 : one; av1 = m < 10 ? av1 : one;
      const float bv0 = S[(10 + m) * TE_STRIDE + 4 * s4 + kq], bv1 = S[(10 + m) * TE_STRIDE + 4 * s4 + 4 + kq];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av0, (double)bv0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av1, (double)bv1, acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  double* R = (double*)stage;
#pragma unroll
  for (int v = 0; v < 4; v++) R[wv * 256 + (kq + 4 * v) * 16 + m] = acc0[v] + acc1[v];
  if (lane == 0) R[(BA_BLOCK / 64) * 256 + wv] = (double)__popcll(onmask);
  __syncthreads();
  if (threadIdx.x < 92) {
    const int t = threadIdx.x;
    int off;
    if (t < 55) { int r = 0, rem = t; while (rem >= 10 - r) { rem -= 10 - r; r++; } off = r * 16 + r + rem; }
    else if (t < 85) off = ((t - 55) / 3) * 16 + 10 + (t - 55) % 3;
    else if (t < 88) off = 10 * 16 + 13 + (t - 85);
    else if (t < 91) off = 11 * 16 + 13 + (t - 88);
    else off = (BA_BLOCK / 64) * 256;   // count slots follow the tiles
    double s = R[off];
#pragma unroll
    for (int w = 1; w < BA_BLOCK / 64; w++) s += R[off + (t < 91 ? w * 256 : w)];
    gst(B.top_part + (size_t)chunk * 92 + t, s);
  }
}

// One workgroup per chunk of <=256 residuals of ONE (host,target) pair.  mode: 0 active, 1 linearized, 2 marginalise.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_accum_top(const BaDev* __restrict__ wins, int mode, const uint8_t* __restrict__ pflag) {
  const BaDev& B = wins[blockIdx.y];
  if (ba_finished(B)) return;
  if ((int)blockIdx.x >= B.nchunks) return;
  const int4 ch = B.chunks[blockIdx.x];
  const int i = ch.y + threadIdx.x;
  const int S = B.nrp;
  bool on = (int)threadIdx.x < ch.z;
  if (on) {
    const uint8_t lin = B.r_lin[i] & 1, act = B.r_act[i];
    if (mode == 0) on = !lin && act;
    else if (mode == 1) on = lin && act;
    else on = act && pflag[B.r_point[i]];
  }
  __shared__ float red[TE_LDS_FLOATS];
  TOP_OPERANDS_DECLARE();
  if (on) {
    float jl[76];
    load_J(B.J[B.r_jsel[i]], S, i, jl);
    float resApprox[8];
    if (mode == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) resApprox[k] = JV(J_RESF + k);
    } else if (mode == 2) {
#pragma unroll
      for (int k = 0; k < 8; k++) resApprox[k] = B.r_toZero[k * S + i];
    } else {
      const float* dp = B.t_adHTdelta + (size_t)ch.x * 8;
      float dx, dy;
      jac_delta(jl, dp, B.t_cdelta, B.p_delta[B.r_point[i]], dx, dy);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        float rtz = B.r_toZero[k * S + i];
        rtz = rtz + JV(J_IDX0 + k) * dx;
        rtz = rtz + JV(J_IDX1 + k) * dy;
        rtz = rtz + JV(J_AB0 + k) * dp[6];
        rtz = rtz + JV(J_AB1 + k) * dp[7];
        resApprox[k] = rtz;
      }
    }
    float JI_r0 = 0, JI_r1 = 0, Jab_r0 = 0, Jab_r1 = 0, rr = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      JI_r0 += resApprox[k] * JV(J_IDX0 + k);
      JI_r1 += resApprox[k] * JV(J_IDX1 + k);
      Jab_r0 += resApprox[k] * JV(J_AB0 + k);
      Jab_r1 += resApprox[k] * JV(J_AB1 + k);
      rr += resApprox[k] * resApprox[k];
    }
    float* rec = B.r_rec + (size_t)B.r_orig[i] * 16;
    TOP_OPERANDS_FILL(JI_r0, JI_r1, Jab_r0, Jab_r1, rr, rec[RR_BD], rec[RR_HDD], (rec + RR_HCD));
  }
  TOP_OPERANDS_EMIT(on, red, blockIdx.x);
}

// ------------------------------------------------------------------ fused linearize + applyRes + accumulate (mode 0)
// FullSystem::optimize with setting_forceAceptStep (the reference default, settings.cpp:53) always applies
// the fresh linearization, so linearizeAll -> applyRes_Reductor(true) -> accumulateAF of the next
// solveSystemF can run back to back on the same residual while its Jacobian is still in registers:
// one workgroup per chunk of one (host,target) pair, J is written to HBM only when MATERIALIZE
// (the reference API keeps RawResidualJacobian; the solver itself never reads it again).
// Linearized residuals are untouched (their accumulation is the separate mode-1 pass).
// Workgroups per CU: four, with and without the Jacobian stores (102 / 101 VGPRs, 40 KB of LDS each); the register count rests on the
// per-pixel sums being completed pixel by pixel (linearize_coop), tests/test_lin_isa_cpu.py holds it.
// The 32 taps of a residual come in through the cooperative quad gather (linearize_coop).  (Rounds 1-4 kept two more gathers for A/B — one
// residual's taps on one lane, and LDS-DMA rounds; both lost or tied, profiles/README.md.)  One chunk per workgroup: a persistent workgroup
// that requested the next chunk's inputs under the current one's work was 26-28 % slower (spills at three waves per SIMD,
// profiles/r06_lin_pk_ab.txt).
// The kernel asks for everything as early as its address is known and waits once per batch, so that a wave waits for few memory round
// trips one after the other (tools/isa_waits.py prints the waits of a listing; tests/test_lin_isa_cpu.py
// holds them): the wave-uniform tables through the scalar cache at entry; the residual's eight scalars in one round trip; the point's
// 80 bytes in a second, ahead of the projection's early exits; four batches of eight tap loads, one wait each; nothing behind the
// Jacobian stores — no value this lane stored is read back, and the record's address is known since the first round trip.  No access
// is a flat_ one (ba_kernels.h: gld / gst / uld), so these waits count memory alone.  How the gain over the former kernel splits between
// these waits and the fourth workgroup per CU has not been measured (profiles/lin_waits_ab.txt).
// The workgroup barriers behind the linearisation exchange data through LDS only (the gather stage handed over to the reduction's panels, the
// energy sum, the waves' tiles); the first stands behind the record stores, which touch no LDS.
template <bool MATERIALIZE>
__global__ __launch_bounds__(BA_BLOCK, 4) void k_ba_lin_fused(const BaDev* __restrict__ wins, int nwin, int max_chunks) {
  // XCD-aware mapping (as k_track_eval, tracker.hip): linear workgroup id L runs on XCD (L % 8); every chunk of window `win` gets the same
  // residue, so ONE L2 serves the window's points (a point's 80 bytes are read by its ~6.5 residuals, which sit in different chunks) and
  // the image lines that the chunks of one target share.  The grid is ceil(nwin / 8) * 8 * max_chunks workgroups: (win, chunk) <-> L is
  // one-to-one, and the ids of the windows that round nwin up to a multiple of 8 leave here.  Speed only; any placement is correct.
  // (-2.0 % on the 256-window step, alone and on top of the 5x2 tiles: profiles/lin_tiles_ab.txt)
  const int L = blockIdx.x;
  const int win = ((L >> 3) / max_chunks) * 8 + (L & 7);
  const int chunk = (L >> 3) % max_chunks;
  if (win >= nwin) return;
  // by-value copy: the descriptor's fields come in through s_load and stay in SGPRs.  Its pointers are still generic ones to the compiler;
  // every access below says "global" (gld / gst) or "uniform" (uld) itself, ba_kernels.h
  const BaDev B = wins[win];
  if (ba_finished_lin(B)) return;
  if (chunk >= B.nchunks) return;
  constexpr int STAGE_FLOATS = (BA_BLOCK / 64) * CG_WAVE_FLOATS;
  constexpr int RED_FLOATS = TE_LDS_FLOATS > STAGE_FLOATS ? TE_LDS_FLOATS : STAGE_FLOATS;
  __shared__ float red[RED_FLOATS];    // the gather stage of the linearisation, then the MFMA panels of the reduction
  double* const lds = (double*)red;    // (the energy reduction runs between the two uses; 40 KB in all = four workgroups per CU)
  // One (host,target) pair per workgroup: the chunk, the pair's 27 precalc floats, the target's image pointer and the two frames' thresholds
  // are wave-uniform and written by earlier kernels only — requested once, here, through the scalar cache
  const i32x4 ch = uld((const i32x4*)(B.chunks + chunk));
  const int pair = ch.x;
  const int h = pair % B.nf, t = pair / B.nf;
  float pre[27];
  {
    const float* prep = B.t_precalc + (size_t)(h * B.nf + t) * 27;
#pragma unroll
    for (int k = 0; k < 27; k++) pre[k] = uld(prep + k);
  }
  const tap_rsrc_t img = __builtin_amdgcn_make_buffer_rsrc((void*)uld((const unsigned long long*)B.t_img + t), 0, TAP_RANGE, TAP_RSRC_FLAGS);
  const float th = fmaxf(uld(B.t_frameTH + h), uld(B.t_frameTH + t));
  const int i = ch.y + threadIdx.x;
  TOP_OPERANDS_DECLARE();
  bool on = false;
  // first round trip: everything the kernel reads of the residual itself
  uint8_t lin, st, jsel, act_old;
  int pt, orig;
  float energy_old, newEnergy_old;
  {
    const int il = (int)threadIdx.x < ch.z ? i : ch.y;   // lanes past the chunk's end read its first residual's (a chunk is never empty): no branch, no extra line
    lin = gld(B.r_lin + il); st = gld(B.r_state + il); pt = gld(B.r_point + il); jsel = gld(B.r_jsel + il); orig = gld(B.r_orig + il);
    energy_old = gld(B.r_energy + il); newEnergy_old = gld(B.r_newEnergy + il); act_old = gld(B.r_act + il);
  }
  vm_wait_all();
  const bool live = (int)threadIdx.x < ch.z && !lin;
  if (!live) st = 1;
  // second round trip: the point's 80 bytes, ahead of the projection and its early exits
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 pg = z4, c0 = z4, c1 = z4, w0 = z4, w1 = z4;
  if (st != 1) {
    pg = gld((const f32x4*)B.p_geo + pt);
    c0 = gld((const f32x4*)(B.p_color + (size_t)pt * 8)); c1 = gld((const f32x4*)(B.p_color + (size_t)pt * 8 + 4));
    w0 = gld((const f32x4*)(B.p_weights + (size_t)pt * 8)); w1 = gld((const f32x4*)(B.p_weights + (size_t)pt * 8 + 4));
  }
  float jl[76];
  float rs5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int ns = 1;
  const float ef = linearize_coop<MATERIALIZE, 2>(B, i, live, st != 1, pre, img, th, pg, c0, c1, w0, w1, jsel, energy_old, jl, ns, rs5,
                                                  red + (threadIdx.x >> 6) * CG_WAVE_FLOATS);
  double e = (double)ef;
  if (live) {
    float* rec = B.r_rec + (size_t)orig * 16;
    // the 64-byte record of this residual (BaDev::r_rec): written once, whole, at the end (four 16-byte stores of one half line)
    float o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rbd = 0.f, rhdd = 0.f, rhcd[4] = {0.f, 0.f, 0.f, 0.f};
    uint8_t act = 0;
    if (st != 1) {  // applyRes(true): OOB is sticky
      if (ns == 0) {
        act = 1;
        if (MATERIALIZE && !B.jfix) gst(B.r_jsel + i, (uint8_t)(jsel ^ 1));
        JAC_TAKE_DATA(o8);
      }
      gst(B.r_act + i, act);
      gst(B.r_state + i, (uint8_t)ns);
      gst(B.r_energy + i, ns != 1 ? ef : newEnergy_old);   // r_newEnergy[i]: this launch's where the linearisation ran to its end, else the one it left
      on = act != 0;
    } else {
      on = act_old != 0;   // (an OOB residual is never active)
    }
    if (on) {   // AccumulatedTopHessianSSE::addPoint<0>, resApprox = resF
      const float JI_r0 = rs5[0], JI_r1 = rs5[1], Jab_r0 = rs5[2], Jab_r1 = rs5[3], rr = rs5[4];
      TOP_OPERANDS_FILL(JI_r0, JI_r1, Jab_r0, Jab_r1, rr, rbd, rhdd, rhcd);
    }
    if (st != 1) {   // (a sticky-OOB residual keeps the records its last applyRes wrote: flags 0)
      gst((f32x4*)rec, (f32x4){o8[0], o8[1], o8[2], o8[3]});
      gst((f32x4*)(rec + 4), (f32x4){o8[4], o8[5], o8[6], o8[7]});
      gst((f32x4*)(rec + 8), (f32x4){rbd, rhdd, rhcd[0], rhcd[1]});
      gst((f32x4*)(rec + 12), (f32x4){rhcd[2], rhcd[3], (float)act, 0.f});
    }
  }
  __syncthreads();   // the reduction below reuses the stage of all waves (behind the record stores: they touch no LDS and need not wait here)
  e = block_sum_d(e, lds);
  if (threadIdx.x == 0) gst(B.e_part + chunk, e);
  __syncthreads();
  TOP_OPERANDS_EMIT(on, red, chunk);
}
#undef TOP_OPERANDS_EMIT
#undef TOP_OPERANDS_FILL
#undef TOP_OPERANDS_DECLARE

// ------------------------------------------------------------------ linearised energy (EnergyFunctional::calcLEnergyPt, EnergyFunctional.cpp:354-417)
// sum over linearized & active residuals of (2*res_toZeroF + J*delta) * J*delta, plus deltaF^2 * priorF per point.
// grid.x = nchunks (one (host,target) pair each: adHTdeltaF is uniform) + point blocks; one float partial per workgroup.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_lenergy(const BaDev* __restrict__ wins, float* __restrict__ out, int out_stride = 0 /* floats between the windows' partials */,
                                                         int cond = 0) {
  const BaDev& B = wins[blockIdx.y];
  if (ba_finished_lin(B) || ba_gate_skip(B, cond)) return;
  if ((int)blockIdx.x >= B.nchunks + (B.np + BA_BLOCK - 1) / BA_BLOCK) return;
  out += (size_t)blockIdx.y * out_stride;
  float e = 0.f;
  if ((int)blockIdx.x < B.nchunks) {
    const int4 ch = B.chunks[blockIdx.x];
    const int i = ch.y + threadIdx.x;
    if ((int)threadIdx.x < ch.z && (B.r_lin[i] & 1) && B.r_act[i]) {
      float jl[76];
      load_J(B.r_jsel[i] ? B.J[1] : B.J[0], B.nrp, i, jl);
      const float* dp = B.t_adHTdelta + (size_t)ch.x * 8;
      float dx, dy;
      jac_delta(jl, dp, B.t_cdelta, B.p_delta[B.r_point[i]], dx, dy);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        float Jdelta = JV(J_IDX0 + k) * dx;
        Jdelta = Jdelta + JV(J_IDX1 + k) * dy;
        Jdelta = Jdelta + JV(J_AB0 + k) * dp[6];
        Jdelta = Jdelta + JV(J_AB1 + k) * dp[7];
        float r0 = B.r_toZero[k * B.nrp + i];
        r0 = r0 + r0;
        r0 = r0 + Jdelta;
        e += Jdelta * r0;
      }
    }
  } else {
    const int p = ((int)blockIdx.x - B.nchunks) * BA_BLOCK + threadIdx.x;
    if (p < B.np) { const float d = B.p_delta[p]; e = d * d * B.p_prior[p]; }
  }
  __shared__ float red[BA_BLOCK / 64];
  e = wave_sum(e);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) { float s = 0; for (int w = 0; w < BA_BLOCK / 64; w++) s += red[w]; out[blockIdx.x] = s; }
}

// fold chunk partials per pair (fixed order) into the packed accumulator; one 128-thread workgroup per pair
__device__ __forceinline__ void fold_top_body(const BaDev& B, int pair, int which /*0 = A, 1 = L*/, int tid) {
  if (pair >= B.nf * B.nf) return;
  const int cb = B.pair_chunk_beg[pair], ce = B.pair_chunk_beg[pair + 1];
  float* out = B.accum + (which ? acc_off_topL(B.nf) : acc_off_topA(B.nf)) + (size_t)pair * 91;
  if (tid < 91) {
    double s = 0;
    for (int ck = cb; ck < ce; ck++) s += B.top_part[(size_t)ck * 92 + tid];
    out[tid] = (float)s;
  }
  if (pair == 0 && tid == 127) {
    double s = 0;
    for (int ck = 0; ck < B.nchunks; ck++) s += B.top_part[(size_t)ck * 92 + 91];
    B.accum[acc_off_nres(B.nf) + which] = (float)s;
  }
}
__device__ __forceinline__ void zero_topL_body(const BaDev& B, int pair, int tid) {
  if (pair >= B.nf * B.nf) return;
  if (tid < 91) B.accum[acc_off_topL(B.nf) + (size_t)pair * 91 + tid] = 0.f;
  if (pair == 0 && tid == 127) B.accum[acc_off_nres(B.nf) + 1] = 0.f;
}
__global__ __launch_bounds__(128) void k_ba_fold_top(const BaDev* __restrict__ wins, int which) { if (ba_finished(wins[blockIdx.y])) return; fold_top_body(wins[blockIdx.y], blockIdx.x, which, threadIdx.x); }
__global__ __launch_bounds__(128) void k_ba_zero_topL(const BaDev* __restrict__ wins) { if (ba_finished(wins[blockIdx.y])) return; zero_topL_body(wins[blockIdx.y], blockIdx.x, threadIdx.x); }

}  // namespace sdso
