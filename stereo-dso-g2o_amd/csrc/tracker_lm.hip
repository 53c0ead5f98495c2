// The resident driver of trackNewestCoarse: the LM step on one wave and the clustered kernel k_track_lm (part of tracker.hip).
// ---- the LM step of the resident driver, by the 64 lanes of wave 0 ------------------------------------------------------------
__device__ __forceinline__ double lm_readlane(double v, int src) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, src), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), src);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// value of lane 8 (lane / 8) + k: ds_swizzle_b32 in bit mode (and 0x18, or k) — a broadcast inside every group of eight lanes, no address register
template <int K>
__device__ __forceinline__ double lm_bcast8_c(double v) {
  const unsigned long long u = __double_as_longlong(v);
  constexpr int pat = 0x18 | (K << 5);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)u, pat), hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(u >> 32), pat);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lm_bcast8(double v, int k) {   // k is a constant after unrolling
  switch (k) {
    case 0: return lm_bcast8_c<0>(v); case 1: return lm_bcast8_c<1>(v); case 2: return lm_bcast8_c<2>(v); case 3: return lm_bcast8_c<3>(v);
    case 4: return lm_bcast8_c<4>(v); case 5: return lm_bcast8_c<5>(v); case 6: return lm_bcast8_c<6>(v); default: return lm_bcast8_c<7>(v);
  }
}
// x = A^-1 rhs for the leading n x n block (n <= 8) of a symmetric A: the algorithm of solveLdltSmall / Eigen::LDLT (symmetric pivoting
// on the first largest |diagonal| of the not yet eliminated positions, read from the INPUT matrix as Eigen's left-looking loop does), with
// the matrix spread over the wave — lane 8i + j holds A(i,j), every lane of row i holds rhs(i) — and every element updated by the
// expression the sequential code uses (the upper triangle mirrors the lower one: its lanes evaluate the lower element's expression with
// the roles swapped).  Because the pivot search only ever reads the input diagonal, the whole pivot order is known before the first
// elimination: every lane replays the eight selections on the eight diagonal values (wave-uniform arithmetic), the matrix is exchanged
// ONCE, and the eight elimination steps are readlane -> divide -> two broadcasts -> update (the forward substitution rides along: same
// terms, same order as the sequential loop).  The division by D runs on all rows at once.  All lanes return with the same x[0..7].
// (History: a single lane walking these 64 doubles through LDS took ~19 us per solve; exchanging per step 4.2 us; this form 2.3 us.)
__device__ __forceinline__ void lm_wave_ldlt(double a, double rhs, int n, double* __restrict__ xs /* LDS, 8 doubles: x by ORIGINAL index */) {
  const int lane = threadIdx.x & 63, i = lane >> 3, j = lane & 7;
  // everything outside the leading n x n block is zero: a zero pivot leaves its column alone and contributes nothing anywhere, so the
  // eight steps below run unconditionally — straight-line code, selects instead of branches (the branchy form was 2 500 instructions)
  a = (i < n && j < n) ? a : 0.0;
  rhs = i < n ? rhs : 0.0;
  double dg[8];
  int perm[8];
#pragma unroll
  for (int m = 0; m < 8; m++) { dg[m] = fabs(lm_readlane(a, m * 9)); perm[m] = m; }
#pragma unroll
  for (int k = 0; k < 7; k++) {
    double best = dg[k];
    int p = k;
#pragma unroll
    for (int m = k + 1; m < 8; m++) { const bool gt = dg[m] > best; best = gt ? dg[m] : best; p = gt ? m : p; }
    const int pk = perm[k];
    int pp = pk;
#pragma unroll
    for (int m = k + 1; m < 8; m++) { const bool is = m == p; pp = is ? perm[m] : pp; dg[m] = is ? dg[k] : dg[m]; perm[m] = is ? pk : perm[m]; }
    perm[k] = pp;
    dg[k] = best;
  }
  int si = perm[0], sj = perm[0];
#pragma unroll
  for (int m = 1; m < 8; m++) { si = i == m ? perm[m] : si; sj = j == m ? perm[m] : sj; }
  a = __shfl(a, si * 8 + sj, 64);
  double y = __shfl(rhs, si * 8, 64);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double dk = lm_readlane(a, k * 9);
    const double yk = lm_readlane(y, k * 8);
    const bool nz = dk != 0.0;                      // a zero pivot leaves its column as it is
    const double l = nz ? a / dk : a;               // column k below the diagonal: L(i,k)
    const double lik = lm_bcast8(l, k), ljk = __shfl(l, j * 8 + k, 64);
    const bool lower = i >= j;                      // the upper triangle mirrors the lower element (j,i): the same expression with the roles swapped
    const double an = a - ((lower ? lik : ljk) * dk) * (lower ? ljk : lik);   // A(i,j) -= (l_ik d_k) A(j,k)
    a = (nz && i > k && j > k) ? an : a;
    a = (nz && j == k && i > k) ? l : a;
    y = i > k ? y - lik * yk : y;                   // L z = rhs, term k of row i
  }
  // D, on every row at once
  double dmine = lm_readlane(a, 0);
#pragma unroll
  for (int m = 1; m < 8; m++) { const double d = lm_readlane(a, m * 9); dmine = i == m ? d : dmine; }
  const double w = dmine != 0.0 ? y / dmine : 0.0;
  // L^T x = w, every lane redundantly (values by v_readlane at fixed lanes): same summation order as the sequential code (the terms past n are 0 * 0)
  double yv[8];
#pragma unroll
  for (int r = 0; r < 8; r++) yv[r] = lm_readlane(w, r * 8);
#pragma unroll
  for (int r = 6; r >= 0; r--) {
    double sacc = yv[r];
#pragma unroll
    for (int c = r + 1; c < 8; c++) sacc -= lm_readlane(a, c * 8 + r) * yv[c];
    yv[r] = sacc;
  }
  // position r holds the unknown of original index perm[r]
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 8; r++) xs[perm[r]] = yv[r];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// SE3::exp of host_math.h (expSe3 / expSo3, the same expressions element by element) for a WAVE-UNIFORM tangent: the four
// trigonometric values it needs — sin, cos of theta / 2 and of theta — come from ONE sincos evaluated on two lanes (lane 0: theta / 2,
// lane 1: theta) instead of four calls in a row on one lane; everything else is evaluated by every lane on the same numbers.
__device__ __forceinline__ Se3 lm_exp_se3_wave(const double* xi) {
  const V3 om{{xi[3], xi[4], xi[5]}};
  const double th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
  const double th = std::sqrt(th2);
  double sv, cv;
  sincos((threadIdx.x & 1) ? th : 0.5 * th, &sv, &cv);
  const double s_half = lm_readlane(sv, 0), c_half = lm_readlane(cv, 0), s_full = lm_readlane(sv, 1), c_full = lm_readlane(cv, 1);
  double im, re;
  if (th < kSophusEps) {
    const double th4 = th2 * th2;
    im = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4;
    re = 1.0 - 0.5 * th2 + (1.0 / 384.0) * th4;
  } else {
    im = s_half / th;
    re = c_half;
  }
  Se3 T;
  T.R = rotationFromQuat(re, im * om[0], im * om[1], im * om[2]);
  const M3 Om = skew(om);
  const M3 Om2 = mul(Om, Om);
  M3 V;
  if (th < kSophusEps) {
    V = T.R;
  } else {
    const double a = (1.0 - c_full) / (th * th);
    const double b = (th - s_full) / (th * th * th);
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * Om[i] + b * Om2[i];
  }
  T.t = mul(V, V3{{xi[0], xi[1], xi[2]}});
  return T;
}

// wave 0 of k_track_lm, between two evaluations: finalise the sums (calcGSSSE :580-595, calcRes :783-789, the expressions of
// k_track_finalize), take the LM decisions (LmCore::consume_pre), solve for the increment, propose the trial pose
// (LmCore::propose_post) and build the request of the next evaluation (fill_eval) — the serial part of a call, 28 times per call.
// Everything here is WAVE-UNIFORM arithmetic: all 64 lanes evaluate the same scalar expressions on the same numbers (LDS broadcast
// reads), so the loads of a stage are requested together, nothing waits for one lane's chain of LDS round trips, and only the
// stores are lane 0's.  (History: decisions, SE3::exp and fill_eval as scalar code of lane 0 / thread 0 with LmCore in LDS between
// them: 2 150 + 3 830 + 2 150 cycles per evaluation, profiles/r04_lm_stamps.txt.)  The common case — the evaluation is consumed and
// another LM step is proposed on the same level — runs in this form; what ends a level or repeats an evaluation with a doubled
// cut-off (five to ten times per call) goes through LmCore's own methods on lane 0, exactly as the host driver runs them.
// The accepted system lives in the wave's registers — lane 8i + j holds H(i,j) and b(i) — between the evaluations (Hacc / bacc).
// Returns the call's `done`; otherwise `ev`, `s_lvl` and the call's counters are those of the next evaluation.
__device__ __forceinline__ bool lm_wave_step(LmCore& core, const float* F, const int* I, double& Hacc, double& bacc, sdso_track_eval_t& ev,
                                             const float (*s_Ki)[9], const int* s_n, int& s_lvl) {
  const int lane = threadIdx.x & 63;
  const int i = lane >> 3, j = lane & 7;
  // ---- every LDS input of the decision, requested together
  const int nE = I[0], nSat = I[1], nWarp = I[2], nShift = I[3];
  const float f45 = F[45], f46 = F[46], f47 = F[47];
  const int phase = core.phase, lvl = core.lvl, it0 = core.iteration;
  const float lam0 = core.lambda, lcr = core.levelCutoffRepeat;
  const double old0 = core.oldres[0], old1 = core.oldres[1];
  const int maxIt = core.p.maxIterations[lvl];
  double nrm = 0;
#pragma unroll
  for (int r = 0; r < 8; r++) { const double v = core.inc[r]; nrm += v * v; }
  const int npad = (nWarp + 3) & ~3;
  double Hnew, bnew;
  {
    auto scale_of = [](int k) -> double { return k < 3 ? (double)SCALE_XI_ROT : k < 6 ? (double)SCALE_XI_TRANS : k == 6 ? (double)SCALE_A : (double)SCALE_B; };
    const float inv_n = 1.0f / npad;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const float fh = F[lo * 9 - lo * (lo - 1) / 2 + (hi - lo)], fb = F[i * 9 - i * (i - 1) / 2 + (8 - i)];
    double v = npad > 0 ? (double)fh * (double)inv_n : 0.0;
    v *= scale_of(j); v *= scale_of(i);
    Hnew = v;
    double u = npad > 0 ? (double)fb * (double)inv_n : 0.0;
    u *= scale_of(i);
    bnew = u;
  }
  LMS(7);
  double res[6];
  track_res6(f45, f46, f47, nE, nSat, nShift, res);
  // ---- LmCore::consume_pre, the case that proposes another step on this level (uniform); anything else: lane 0, below
  bool fast, take, accept = false;
  float lambda = lam0;
  int iteration = it0;
  if (phase == 0) {
    fast = !(res[5] > 0.6 && lcr < 50) && 0 < maxIt;                                  // :897-904
    take = true; lambda = 0.01f; iteration = 0;
  } else {
    accept = (res[0] / res[1]) < (old0 / old1);                                       // :1004
    take = accept;
    if (accept) lambda *= 0.5;
    else { lambda *= 4; if (lambda < kLambdaExtrapolationLimit) lambda = kLambdaExtrapolationLimit; }
    iteration = it0 + 1;
    fast = std::sqrt(nrm) > 1e-3 && iteration < maxIt;                                // :1022, :927
  }
  int act = 1;
  if (fast) {
    if (lane == 0) {
      if (take) {
#pragma unroll
        for (int r = 0; r < 6; r++) core.oldres[r] = res[r];
      }
      if (phase == 1 && accept) { core.affCur = core.affNew; core.cur = core.Tnew; }
      core.lambda = lambda; core.iteration = iteration;
      core.out.iterations[lvl]++;
    }
  } else {
    int a = 0, t = 0;
    if (lane == 0) { bool tk = false; a = core.consume_pre(res, tk); t = tk ? 1 : 0; }
    act = __builtin_amdgcn_readfirstlane(a);
    take = __builtin_amdgcn_readfirstlane(t) != 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (act) lambda = core.lambda;               // (cannot happen with the predicates above; kept so that the two forms can never disagree silently)
  }
  LMS(8);
  if (act) {
    if (take) { Hacc = Hnew; bacc = bnew; }
    // LmCore::solve_inc on the wave
    const double lam1 = 1 + lambda;
    double a = Hacc;
    if (i == j) a *= lam1;
    const double nb = -bacc;
    const bool fixA = core.p.affineOptModeA < 0, fixB = core.p.affineOptModeB < 0;
    // the full solve, then (when an affine parameter is fixed) the reduced one of :937-964 — ONE copy of the factorisation in the code: the
    // kernel's loop has to stay inside the instruction cache
    double incv[8];
    const int npass = (fixA || fixB) ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < npass; pass++) {
      double am = a, bm = nb;
      int n = 8;
      if (pass == 1) {
        n = (fixA && fixB) ? 6 : 7;
        if (fixA && !fixB) {   // rows / columns 6 <- 7 of the damped matrix, b likewise (:949-964)
          const int si = i == 6 ? 7 : i, sj = j == 6 ? 7 : j;
          am = __shfl(a, si * 8 + sj, 64);
          bm = __shfl(nb, si * 8, 64);
        }
      }
      lm_wave_ldlt(am, bm, n, core.wx);
      double x[8];
#pragma unroll
      for (int r = 0; r < 8; r++) x[r] = core.wx[r];
      if (pass == 0) {
#pragma unroll
        for (int r = 0; r < 8; r++) incv[r] = x[r];
      } else lm_place_reduced(fixA, fixB, x, incv);
    }
    LMS(9);
    // the state the proposal starts from, K[lvl]^-1 and the cut-off of the next request, requested together (lane 0's stores above are
    // behind the wave barrier that ends lm_wave_ldlt); the level's other constants are read from core.p by fill_eval_ki below
    Se3 cur;
#pragma unroll
    for (int r = 0; r < 9; r++) cur.R[r] = core.cur.R[r];
#pragma unroll
    for (int r = 0; r < 3; r++) cur.t[r] = core.cur.t[r];
    const sdso_aff_t affCur = core.affCur;
    float Ki[9];
#pragma unroll
    for (int r = 0; r < 9; r++) Ki[r] = s_Ki[lvl][r];
    const float cutoff = core.p.coarseCutoffTH * core.levelCutoffRepeat;
    // LmCore::propose_post (:966-1000), uniform
    double incScaled[8];
    lm_scale_step(lambda, incv, incScaled);
    const Se3 Tnew = lm_exp_se3_wave(incScaled) * cur;
    sdso_aff_t affNew = affCur;
    affNew.a += incScaled[6];
    affNew.b += incScaled[7];
    sdso_track_eval_t evl;
    fill_eval_ki(core.p, lvl, Ki, Tnew, affNew, cutoff, evl);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 8; r++) core.inc[r] = incv[r];
      core.Tnew = Tnew; core.affNew = affNew;
      core.phase = 1;
      core.reqT = Tnew; core.reqAff = affNew;
      ev = evl;
      core.out.evaluations++;
      core.out.point_evals += s_n[lvl];
    }
    LMS(10);
    return false;
  }
  LMS(10);
  // lane 0 has set the next request itself (a new level, a repeated evaluation) or ended the call
  int done = 0;
  if (lane == 0) {
    done = core.done ? 1 : 0;
    if (!done) {
      fill_eval(core.p, core.lvl, core.reqT, core.reqAff, core.p.coarseCutoffTH * core.levelCutoffRepeat, ev);
      s_lvl = core.lvl;
      core.out.evaluations++;
      core.out.point_evals += s_n[core.lvl];
    }
  }
  return __builtin_amdgcn_readfirstlane(done) != 0;
}

// ---- a CLUSTER of G workgroups per hypothesis --------------------------------------------------------------------------------------
// One CU evaluates a 4 000-point level at the rate its L1 is filled (two 128-byte lines per template point at 64 bytes per clock: the
// point loop of a single workgroup was 55 % of the call).  With G > 1 the hypothesis' points are strided over G workgroups on G CUs (placed
// on ONE XCD: workgroup L runs on XCD L % 8).  EVERY member runs the LM state machine: per evaluation a member publishes its 52 partial
// sums in an LmCluster record in global memory, collects the other members', adds all of them in member order — so every member holds the
// same sums, bit for bit — and takes the same decisions with the same arithmetic: the next request never has to travel.  ONE hand-off per
// evaluation (a leader that gathers the partials and publishes the next request needs two: 0.355 against 0.31 ms per call).
// A partial travels as 64-bit {word, evaluation number} pairs written and polled by single relaxed agent-scope atomics: a reader that sees
// the tag of evaluation e has that evaluation's word — no flag, no fence, one round trip (≈ 0.7 us on one XCD, tools/handoff_bench.hip).
// Two buffers alternate: a member can be one evaluation ahead of a slow reader of its previous partial, never two.  The tags grow from call
// to call (e_base): the records are never cleared between calls — whatever an earlier call left carries a smaller tag.
// Every spin is bounded (a member that never became resident — the device was shared — ends the call with out.evaluations = -1 and
// the host repeats it with G = 1, which needs no co-residency).  Member 0 reports the result.
constexpr int LM_MAXG = 8;
constexpr int LM_SPIN_LIMIT = 1 << 21;
struct LmCluster {                                           // zeroed when allocated; a call's first evaluation is number e_base + 1
  unsigned long long part[2][LM_MAXG][64];
};
__device__ __forceinline__ void lm_put(unsigned long long* slot, unsigned word, int e) {
  __hip_atomic_store(slot, (unsigned long long)word | ((unsigned long long)(unsigned)e << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long lm_get(const unsigned long long* slot) {
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(LM_BLOCK) void k_track_lm(LmJob* __restrict__ jobs, LmCluster* __restrict__ clusters, int nhyp, int G, int spin_limit, int drop_member /* test hook: member G - 1 of every cluster never answers */,
                                                       int solo_n /* levels of at most this many points are not shared */, int e_base /* this call's evaluations carry the tags e_base + 1 .. */) {
  // hypothesis c, member g: for G > 1 the members of a cluster share blockIdx % 8 (one XCD, one L2); speed only, any placement is correct
  int c = blockIdx.x, g = 0;
  if (G > 1) { const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3; g = j % G; c = (j / G) * 8 + xcd; }
  if (c >= nhyp) return;
  if (drop_member && G > 1 && g == G - 1) return;
  LmJob& J = jobs[c];
  LmCluster& C = clusters[c];
  __shared__ __align__(16) unsigned char core_raw[sizeof(LmCore)];     // (LmCore has member initialisers: raw storage, init() sets every field it reads)
  LmCore& core = *reinterpret_cast<LmCore*>(core_raw);
  __shared__ sdso_track_eval_t ev;
  __shared__ float sF[LM_BLOCK / 64][TRK_NF + TRK_NI];
  __shared__ float F[TRK_NF];
  __shared__ int I[TRK_NI];
  __shared__ int s_lvl, s_done, s_abort;
  __shared__ const float4* s_pc[SDSO_PYR_LEVELS];                      // the job's tables, read once (a global round trip per evaluation otherwise)
  __shared__ const float4* s_img[SDSO_PYR_LEVELS];
  __shared__ int s_n[SDSO_PYR_LEVELS];
  const int tid = threadIdx.x, wv = tid >> 6;
  const bool leader = g == 0;
  __shared__ float s_Ki[SDSO_PYR_LEVELS][9];                           // K[lvl]^-1 (fill_eval's inv3f, CoarseTracker.cpp:129-130): per level, not per evaluation
  if (tid < SDSO_PYR_LEVELS) {
    s_pc[tid] = J.pc[tid]; s_img[tid] = J.img[tid]; s_n[tid] = J.n[tid];
    const float K[9] = {J.p.fx[tid], 0, J.p.cx[tid], 0, J.p.fy[tid], J.p.cy[tid], 0, 0, 1};
    float Ki[9];
    inv3f(K, Ki);
    for (int k = 0; k < 9; k++) s_Ki[tid][k] = Ki[k];
  }
  if (tid == 0) {
    core.init(J.p, J.T, J.aff);                 // every member: the same state machine on the same inputs
    s_done = 0; s_abort = 0;
  }
  __syncthreads();
#ifdef SDSO_LM_STAMPS
  if (tid == 0) { for (int k = 0; k < 16; k++) lm_st_acc[k] = 0; lm_st_last = __builtin_amdgcn_s_memtime(); }
#define LMSL(i) do { if (leader) LMS(i); } while (0)
#else
#define LMSL(i) do { } while (0)
#endif
  double Hacc = 0.0, bacc = 0.0;                // wave 0: the accepted system (lm_wave_step)
  float4 qc[LM_UNROLL];                         // this thread's template points of level qlvl
  int qlvl = -1;
#pragma unroll
  for (int u = 0; u < LM_UNROLL; u++) qc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  // A level whose points fit ONE trip of one workgroup (LM_UNROLL points per thread: the coarse levels, more than half of a call's
  // evaluations) is evaluated by every member in full, in the single workgroup's order: the members hold the same sums without the
  // exchange — which costs more (5 k cycles at G = 8) than those points do.  solo_n == 0 (SDSO_TRK_LM_SOLO=0): every level is shared.
  int first = g * LM_BLOCK + tid, stride = G * LM_BLOCK;
  // every trip is one evaluation; the loop ends for all threads together (the flags are read behind a barrier)
  if (tid == 0) {                               // the first request; every later one is built by wave 0 at the end of lm_wave_step
    fill_eval(core.p, core.lvl, core.reqT, core.reqAff, core.p.coarseCutoffTH * core.levelCutoffRepeat, ev);
    s_lvl = core.lvl;
    core.out.evaluations++;
    core.out.point_evals += s_n[core.lvl];
  }
  __syncthreads();
  int shared_evals = 0;
  for (int e = 1; e <= 1024; e++) {
    LMSL(0);
    const int lvl = s_lvl, n = s_n[lvl];
    const bool shared_lvl = G > 1 && n > solo_n;
    if (lvl != qlvl) {                          // (uniform) first evaluation on this level: the points move into registers
      first = shared_lvl ? g * LM_BLOCK + tid : tid; stride = shared_lvl ? G * LM_BLOCK : LM_BLOCK;
      const float4* __restrict__ pc = s_pc[lvl];
      if (first < n) {
#pragma unroll
        for (int u = 0; u < LM_UNROLL; u++) { const int i = first + u * stride; qc[u] = pc[i < n ? i : first]; }
      }
      qlvl = lvl;
    }
    TrackLaneSums S;
    track_accumulate<false, true, LM_UNROLL>(ev, s_pc[lvl], s_img[lvl], n, first, stride, nullptr, S, qc);
    LMSL(3);
    {   // the four counters ride along as floats (exact: they stay far below 2^24), so one 52-value row reduction covers everything
      float v52[TRK_NF + TRK_NI];
#pragma unroll
      for (int k = 0; k < 45; k++) v52[k] = S.acc[k];
      v52[45] = S.E; v52[46] = S.sT; v52[47] = S.sRT;
      v52[48] = (float)S.nE; v52[49] = (float)S.nSat; v52[50] = (float)S.nWarp; v52[51] = (float)S.nShift;
      wave_reduce_rows<TRK_NF + TRK_NI>(v52, [&](int k, float sum) { sF[wv][k] = sum; });
    }
    LMSL(4);
    __syncthreads();
    LMSL(5);
    float mine = 0.f;
    if (tid < TRK_NF + TRK_NI) {                // fixed order over the waves: run-to-run reproducible
      mine = sF[0][tid];
#pragma unroll
      for (int w = 1; w < LM_BLOCK / 64; w++) mine += sF[w][tid];
    }
    if (shared_lvl && tid < TRK_NF + TRK_NI) {  // publish this member's partial, collect the others', add all of them in member order
      unsigned long long (*buf)[64] = C.part[shared_evals & 1];   // (alternating over the SHARED evaluations: between two uses of a buffer lies an exchange on the other one)
      const float own = mine;
      lm_put(&buf[g][tid], __float_as_uint(own), e_base + e);
      unsigned long long v[LM_MAXG];
      bool all = false;
      for (int spins = 0; spins < spin_limit && !all; spins++) {
        all = true;
#pragma unroll
        for (int m = 0; m < LM_MAXG; m++)
          if (m < G && m != g) { v[m] = lm_get(&buf[m][tid]); all = all && (int)(v[m] >> 32) == e_base + e; }
        if (!all) __builtin_amdgcn_s_sleep(1);
      }
      if (!all) s_abort = 1;
      float tot = 0.f;
#pragma unroll
      for (int m = 0; m < LM_MAXG; m++) if (m < G) tot = m == 0 ? (g == 0 ? own : __uint_as_float((unsigned)v[0])) : tot + (m == g ? own : __uint_as_float((unsigned)v[m]));
      mine = tot;
    }
    if (shared_lvl) shared_evals++;
    if (tid < TRK_NF) F[tid] = mine; else if (tid < TRK_NF + TRK_NI) I[tid - TRK_NF] = (int)mine;
    __syncthreads();
    if (s_abort) {                              // a member never answered (every member notices): member 0 gives the call back to the host
      if (leader && tid == 0) { J.out = core.out; J.out.evaluations = -1; J.trace.n = 0; }
      return;
    }
    LMSL(6);
    if (wv == 0) { const bool d = lm_wave_step(core, F, I, Hacc, bacc, ev, s_Ki, s_n, s_lvl); if (tid == 0) s_done = d ? 1 : 0; }
    __syncthreads();
    LMSL(11);
    if (s_done) break;                          // (every member reaches the same verdict)
  }
#undef LMSL
  if (leader && tid == 0) {
    J.out = core.out;
    J.trace.n = core.trace.n;
    for (int e = 0; e < core.trace.n; e++) {
      J.trace.lvl[e] = core.trace.lvl[e]; J.trace.res[e] = core.trace.res[e];
      for (int k = 0; k < 3; k++) J.trace.flow[e][k] = core.trace.flow[e][k];
    }
    if (core.wrote_final) { J.T = core.T_final; J.aff = core.aff_final; }
#ifdef SDSO_LM_STAMPS
    for (int k = 0; k < 9; k++) J.T.R[k] = (double)lm_st_acc[k];
    for (int k = 0; k < 3; k++) J.T.t[k] = (double)lm_st_acc[9 + k];
#endif
  }
}
