// A part of g2o_factors.hip: sdso_g2o_lba_optimize, FullSystem::optimize as the fork compiles it (FullSystemOptimize.cpp:402-868).
//
// Every idepth vertex belongs to one edge (:506-512) and the target pose is a constant (dso_g2o_edge.cpp:23), so with
//   Jp = the edge's 8 x 12 Jacobian over [pose 6 | photometric 2 | camera 4], jd = its 8 x 1 idepth column, e its error, rho1 its Huber weight
// the system g2o's block solver builds is, per host frame, A = sum rho1 [Jp|e]^T [Jp|e] (13 x 13), and per edge the record
//   w = rho1 Jp^T jd (12), bl = -rho1 jd^T e, hll = rho1 jd^T jd
// whose Schur complement at lambda is, per host, S = sum [w|bl]^T [w|bl] / (hll + lambda).  The reduced system is block-arrow (8 x 8 per
// host, 8 x 4 to the camera, 4 x 4 camera): at most 68 unknowns, solved on the host with solveLdlt.  Back-substitution
// xl = (bl - w . xp) / (hll + lambda) runs inside the trial's evaluation kernel.
//
// Residuals are sorted host-major on the way up (a stable counting sort on the host; results are un-permuted on the way down), so a
// host's edges are one range and every sum below is a per-workgroup partial over a fixed range, folded in a fixed order: no atomics on
// floating-point values, bit-identical reruns.
//   k_lba_opt_eval    computeActiveErrors at the current or at the tentative estimate (+ back-substitution); robust chi2, landmark scale
//   k_lba_opt_lin     linearizeOplus + the quadratic form: per-edge records, per-host A; 256 pixel rows are staged in LDS and 2 x 91
//                     threads each own one entry of the upper triangle
//   k_lba_opt_schur   per-host S at lambda, the same entry-per-thread scheme over the records
//   k_lba_opt_fold    partials -> sums, fixed order
//   k_lba_opt_count   active edges per host
// The control flow is csrc/g2o_lm.h on the host, as in sdso_g2o_track_newest_coarse.

namespace sdso {

constexpr int kLbaEnt = 91;          // upper triangle of 13 x 13
constexpr int kLbaRec = 14;          // w 12, bl, hll
constexpr int kLbaEvalBlocks = 128;  // partials of k_lba_opt_eval
constexpr int kLbaLinChunks = 16;    // workgroups per host in k_lba_opt_lin; each writes two partials
constexpr int kLbaScChunks = 16;     // workgroups per host in k_lba_opt_schur

template <class DevT>
struct LbaOptT {
  DevT L;                      // sorted arrays; pair tables, cam and idepth of the estimate the launch evaluates
  const int* hstart;           // nf + 1: the range of every host
  const double* idepth_cur;    // current estimate (the trial adds its increment to it)
  double* idepth_trial;        // tentative estimate, written by the trial
  uint8_t* active;
  uint8_t* level;              // sticky: 1 once any computeError ran setLevel(1)
  double* rec;                 // nr * 14
  const double* x;             // nf * 8 + 4 pose / photometric / camera increments of the trial, by frame index
  double lambda;
  double* part;                // partial sums of the launch
};
typedef LbaOptT<LbaDev> LbaOpt;

__device__ __forceinline__ double group_sum8(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// mode 0: the build-time computeError (FullSystemOptimize.cpp:539) — fixes the active set; 1: computeActiveErrors at the current estimate,
// per-residual results written; 2: at the tentative estimate current + x, nothing but the sums and the tentative idepth written
// (the bodies are stated once: the kernels below take O as a launch argument, those of g2o_lba_resident.hip build it from the job's control block)
template <int MODE, class OptT>
__device__ __forceinline__ void lba_opt_eval_body(const OptT& O) {
  const auto& L = O.L;
  const int idx = threadIdx.x & 7, lane = threadIdx.x & 63, base = lane & ~7, wv = threadIdx.x >> 6;
  double chi = 0, scale = 0;
  for (int g0 = blockIdx.x * 32; g0 < L.nr; g0 += gridDim.x * 32) {
    const int ri = g0 + (threadIdx.x >> 3);
    const bool live = ri < L.nr;
    const int rr = live ? ri : 0;
    const int h = L.host[rr], tg = L.target[rr];
    bool act = MODE == 0 ? true : (live && O.active[rr] != 0);
    double idepth = O.idepth_cur[rr];
    if constexpr (MODE == 2) {
      double xl = 0;
      if (act) {
        const double* rc = O.rec + (size_t)rr * kLbaRec;
        double s = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) s += rc[k] * O.x[h * 8 + k];
#pragma unroll
        for (int k = 0; k < 4; k++) s += rc[8 + k] * O.x[L.nf * 8 + k];
        const double d = rc[13] + O.lambda;
        xl = d != 0 ? (rc[12] - s) / d : 0;
        if (idx == 0) scale += xl * (O.lambda * xl + rc[12]);   // computeScale, the landmark part
      }
      idepth = idepth + xl;                                     // VertexInverseDepthDSO::oplusImpl, dso_g2o_vertex.cpp:56-58
      if (live && idx == 0) O.idepth_trial[ri] = idepth;
    }
    const LbaPix P = lba_pixel<false>(L, rr, idx, h, tg, idepth);
    const LbaGroup G = lba_group(P, base);
    const LbaEdge E = lba_edge(G, fmaxf(L.frameEnergyTH[h], L.frameEnergyTH[tg]));
    const double ek = E.zero ? 0. : P.e;
    const double e2 = group_sum8(ek * ek);
    if (!live) continue;
    if constexpr (MODE == 0) act = E.level == 0;
    if (idx == 0) {
      if constexpr (MODE == 0) { O.active[ri] = act ? 1 : 0; O.level[ri] = E.level; }
      else if (E.level) O.level[ri] = 1;
      if constexpr (MODE != 2) {
        L.state[ri] = E.state;
        L.energy[ri * 2] = E.energy[0]; L.energy[ri * 2 + 1] = E.energy[1];
        L.cpt[ri * 3] = E.cpt[0]; L.cpt[ri * 3 + 1] = E.cpt[1]; L.cpt[ri * 3 + 2] = E.cpt[2];
      }
      if (act) {   // g2o's RobustKernelHuber, as at k_g2o_track_lin
        const double delta = kHuberTH, dsqr = delta * delta;
        chi += e2 <= dsqr ? e2 : 2 * sqrt(e2) * delta - dsqr;
      }
    }
  }
  __shared__ double sm[4][2];
  const double s0 = wave_sum(chi), s1 = wave_sum(scale);
  if (lane == 0) { sm[wv][0] = s0; sm[wv][1] = s1; }
  __syncthreads();
  if (threadIdx.x < 2) O.part[blockIdx.x * 2 + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}
template <int MODE>
__global__ __launch_bounds__(256) void k_lba_opt_eval(LbaOpt O) { lba_opt_eval_body<MODE>(O); }

// entry `ent` of the upper triangle, row-major: (i, j), i <= j < 13
__device__ __forceinline__ void lba_entry(int ent, int& i, int& j) {
  i = 0;
  int k = ent;
  while (k >= 13 - i) { k -= 13 - i; i++; }
  j = i + k;
}

// grid (kLbaLinChunks, nf): workgroup (c, h) takes the tiles c, c + kLbaLinChunks, ... of 32 edges of host h
template <class OptT>
__device__ __forceinline__ void lba_opt_lin_body(const OptT& O) {
  const auto& L = O.L;
  const int h = blockIdx.y;
  const int idx = threadIdx.x & 7, lane = threadIdx.x & 63, base = lane & ~7;
  const int e0 = O.hstart[h], e1 = O.hstart[h + 1];
  __shared__ double sm_row[256][13];
  __shared__ double sm_rho[256];
  const int half = threadIdx.x >> 7, ent = threadIdx.x & 127;
  int ei = 0, ej = 0;
  if (ent < kLbaEnt) lba_entry(ent, ei, ej);
  double acc = 0;
  for (int g0 = e0 + blockIdx.x * 32; g0 < e1; g0 += kLbaLinChunks * 32) {
    const int ri = g0 + (threadIdx.x >> 3);
    const bool live = ri < e1;
    const int rr = live ? ri : e0;
    const int tg = L.target[rr];
    const LbaPix P = lba_pixel<true>(L, rr, idx, h, tg, O.idepth_cur[rr]);
    const LbaGroup G = lba_group(P, base);
    const LbaEdge E = lba_edge(G, fmaxf(L.frameEnergyTH[h], L.frameEnergyTH[tg]));
    const bool act = live && O.active[rr] != 0;
    const bool jz = !act || E.jzero || O.level[rr] != 0;   // linearizeOplus returns early: dso_g2o_edge.cpp:131, :183, :194, :204
    const double ek = E.zero ? 0. : P.e;
    const double e2 = group_sum8(ek * ek);
    const double delta = kHuberTH;
    const double rho1 = !act ? 0. : (e2 <= delta * delta ? 1. : delta / sqrt(e2));
    const double jd = jz ? 0. : P.row[8];
    double rec[kLbaRec];
#pragma unroll
    for (int k = 0; k < 8; k++) rec[k] = group_sum8(rho1 * ((jz ? 0. : P.row[k]) * jd));
#pragma unroll
    for (int k = 0; k < 4; k++) rec[8 + k] = group_sum8(rho1 * ((jz ? 0. : P.row[9 + k]) * jd));
    rec[12] = -group_sum8(rho1 * (jd * ek));
    rec[13] = group_sum8(rho1 * (jd * jd));
    if (live && idx == 0) {
#pragma unroll
      for (int k = 0; k < kLbaRec; k++) O.rec[(size_t)ri * kLbaRec + k] = rec[k];
      L.idepth_hessian[ri] = jz ? 0.f : E.ih;
    }
    __syncthreads();   // the previous tile's rows have been consumed
#pragma unroll
    for (int k = 0; k < 8; k++) sm_row[threadIdx.x][k] = jz ? 0. : P.row[k];
#pragma unroll
    for (int k = 0; k < 4; k++) sm_row[threadIdx.x][8 + k] = jz ? 0. : P.row[9 + k];
    sm_row[threadIdx.x][12] = act ? ek : 0.;
    sm_rho[threadIdx.x] = rho1;
    __syncthreads();
    if (ent < kLbaEnt) {
      for (int r = half * 128; r < half * 128 + 128; r++) acc += (sm_rho[r] * sm_row[r][ei]) * sm_row[r][ej];
    }
  }
  if (ent < kLbaEnt) O.part[((size_t)h * (2 * kLbaLinChunks) + blockIdx.x * 2 + half) * kLbaEnt + ent] = acc;
}
__global__ __launch_bounds__(256) void k_lba_opt_lin(LbaOpt O) { lba_opt_lin_body(O); }

// grid (kLbaScChunks, nf), 128 threads: workgroup (c, h) takes the c-th slice of host h's records
template <class OptT>
__device__ __forceinline__ void lba_opt_schur_body(const OptT& O) {
  const int h = blockIdx.y;
  const int e0 = O.hstart[h], e1 = O.hstart[h + 1];
  const int per = (e1 - e0 + kLbaScChunks - 1) / kLbaScChunks;
  const int s0 = e0 + blockIdx.x * per, s1 = min(s0 + per, e1);
  __shared__ double sm_rec[128][kLbaRec];
  __shared__ double sm_inv[128];
  const int ent = threadIdx.x;
  int ei = 0, ej = 0;
  if (ent < kLbaEnt) lba_entry(ent, ei, ej);
  double acc = 0;
  for (int t0 = s0; t0 < s1; t0 += 128) {
    const int n = min(128, s1 - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < n * kLbaRec; k += 128) sm_rec[k / kLbaRec][k % kLbaRec] = O.rec[(size_t)t0 * kLbaRec + k];
    if (threadIdx.x < n) {
      const double d = O.rec[(size_t)(t0 + threadIdx.x) * kLbaRec + 13] + O.lambda;
      sm_inv[threadIdx.x] = d != 0 ? 1. / d : 0.;
    }
    __syncthreads();
    if (ent < kLbaEnt)
      for (int r = 0; r < n; r++) acc += (sm_rec[r][ei] * sm_inv[r]) * sm_rec[r][ej];
  }
  if (ent < kLbaEnt) O.part[((size_t)h * kLbaScChunks + blockIdx.x) * kLbaEnt + ent] = acc;
}
__global__ __launch_bounds__(128) void k_lba_opt_schur(LbaOpt O) { lba_opt_schur_body(O); }

// out[g][v] = part[g][0][v] + part[g][1][v] + ... in that order; grid = groups, 128 threads
__global__ __launch_bounds__(128) void k_lba_opt_fold(const double* __restrict__ part, int nparts, int nvals, double* __restrict__ out) {
  const int g = blockIdx.x, v = threadIdx.x;
  if (v >= nvals) return;
  double s = 0;
  for (int p = 0; p < nparts; p++) s += part[((size_t)g * nparts + p) * nvals + v];
  out[(size_t)g * nvals + v] = s;
}

// active edges per host; grid nf
__global__ __launch_bounds__(256) void k_lba_opt_count(const int* __restrict__ hstart, const uint8_t* __restrict__ active, int* __restrict__ count) {
  const int h = blockIdx.x;
  __shared__ int sm;
  if (threadIdx.x == 0) sm = 0;
  __syncthreads();
  int c = 0;
  for (int i = hstart[h] + threadIdx.x; i < hstart[h + 1]; i += 256) c += active[i] != 0;
  if (c) atomicAdd(&sm, c);
  __syncthreads();
  if (threadIdx.x == 0) count[h] = sm;
}

// The window as the LM controller sees it (g2o_lm.h): estimates on the host in double except the idepths, which never leave the device.
struct LbaProblem {
  sdso_ctx* ctx;
  const sdso_g2o_lba_window_t* W;
  LbaOpt O;                               // device pointers; the fields a launch varies are set per launch
  int nf, nr;
  Se3 Twh[8], Twh_t[8];
  double aff[8][2], aff_t[8][2], cam[4], cam_t[4];
  int n_active_host[8];
  float* d_tab[2];                        // pair tables {R 9, t 3, ab 2} x nf*nf of the current / tentative estimate
  double* d_idepth[2];
  int cur = 0;                            // which of the two is the current estimate
  double *d_x, *d_part, *d_sum;
  double A[8][kLbaEnt];                   // of the last build()
  double chi2 = 0;

  int tables(const Se3* T, const double (*ab)[2], float* d_dst) {
    float tab[64 * 14];
    const size_t nn = (size_t)nf * nf;
    float *R = tab, *t = tab + nn * 9, *a = tab + nn * 12;
    for (int h = 0; h < nf; h++)
      for (int tg = 0; tg < nf; tg++) {
        const Se3 Tth = se3_from_abi(W->Ttw[tg]) * T[h];                  // dso_g2o_edge.cpp:25
        for (int k = 0; k < 9; k++) R[(h * nf + tg) * 9 + k] = (float)Tth.R[k];
        for (int k = 0; k < 3; k++) t[(h * nf + tg) * 3 + k] = (float)Tth.t[k];
        double o[2];
        affFromTo(W->ab_exposure[h], W->ab_exposure[tg], ab[h][0], ab[h][1], W->target_aff[tg].a, W->target_aff[tg].b, o);   // :86-91
        a[(h * nf + tg) * 2] = (float)o[0]; a[(h * nf + tg) * 2 + 1] = (float)o[1];
      }
    SDSO_HIP(ctx, hipMemcpyAsync(d_dst, tab, sizeof(float) * nn * 14, hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `tab` is on this frame
    return SDSO_OK;
  }
  void point_at(int which, const double* c) {
    const size_t nn = (size_t)nf * nf;
    O.L.pair_R = d_tab[which]; O.L.pair_t = d_tab[which] + nn * 9; O.L.pair_ab = d_tab[which] + nn * 12;
    for (int k = 0; k < 4; k++) O.L.cam[k] = c[k];
  }
  int fold(int groups, int nparts, int nvals, double* host) {
    hipLaunchKernelGGL(k_lba_opt_fold, dim3(groups), dim3(128), 0, ctx->stream, (const double*)d_part, nparts, nvals, d_sum);
    SDSO_HIP(ctx, hipGetLastError());
    SDSO_HIP(ctx, hipMemcpyAsync(host, d_sum, sizeof(double) * groups * nvals, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SDSO_OK;
  }
  // MODE 0 / 1 at the current estimate, 2 at the tentative one
  template <int MODE>
  int eval(double* sums) {
    int rc = MODE == 2 ? tables(Twh_t, aff_t, d_tab[cur ^ 1]) : tables(Twh, aff, d_tab[cur]);
    if (rc) return rc;
    point_at(MODE == 2 ? cur ^ 1 : cur, MODE == 2 ? cam_t : cam);
    O.idepth_cur = d_idepth[cur]; O.idepth_trial = d_idepth[cur ^ 1];
    O.part = d_part;
    const int blocks = std::min(kLbaEvalBlocks, (nr + 31) / 32);
    {
      ProfScope ps(ctx, "k_lba_opt_eval");
      hipLaunchKernelGGL(k_lba_opt_eval<MODE>, dim3(blocks), dim3(256), 0, ctx->stream, O);
    }
    SDSO_HIP(ctx, hipGetLastError());
    return fold(1, blocks, 2, sums);
  }

  int build() {
    point_at(cur, cam);
    O.idepth_cur = d_idepth[cur];
    O.part = d_part;
    {
      ProfScope ps(ctx, "k_lba_opt_lin");
      hipLaunchKernelGGL(k_lba_opt_lin, dim3(kLbaLinChunks, nf), dim3(256), 0, ctx->stream, O);
    }
    SDSO_HIP(ctx, hipGetLastError());
    return fold(nf, 2 * kLbaLinChunks, kLbaEnt, &A[0][0]);
  }
  int trial(double lambda, g2o_lm::TrialEval* t) {
    O.lambda = lambda;
    O.part = d_part;
    {
      ProfScope ps(ctx, "k_lba_opt_schur");
      hipLaunchKernelGGL(k_lba_opt_schur, dim3(kLbaScChunks, nf), dim3(128), 0, ctx->stream, O);
    }
    SDSO_HIP(ctx, hipGetLastError());
    double S[8][kLbaEnt];
    int rc = fold(nf, kLbaScChunks, kLbaEnt, &S[0][0]);
    if (rc) return rc;
    // the reduced system over the hosts that have an active edge, in frame order, then the camera
    int slot[8], nh = 0;
    for (int h = 0; h < nf; h++) slot[h] = n_active_host[h] > 0 ? nh++ : -1;
    const int n = 8 * nh + 4;
    Dense Hr(n);
    std::vector<double> bfull(n, 0.0), bred(n, 0.0), x(n, 0.0);
    for (int h = 0; h < nf; h++) {
      if (slot[h] < 0) continue;
      int ent = 0;
      for (int i = 0; i < 13; i++)
        for (int j = i; j < 13; j++, ent++) {
          const int gi = i < 8 ? 8 * slot[h] + i : 8 * nh + (i - 8);
          if (j == 12) {
            if (i < 12) { bfull[gi] -= A[h][ent]; bred[gi] += -A[h][ent] - S[h][ent]; }
            continue;
          }
          const int gj = j < 8 ? 8 * slot[h] + j : 8 * nh + (j - 8);
          const double v = A[h][ent] - S[h][ent];
          Hr(gi, gj) += v;
          if (gi != gj) Hr(gj, gi) += v;
        }
    }
    for (int k = 0; k < n; k++) Hr(k, k) += lambda;
    t->solved = solveLdlt(Hr, bred, x);
    double xf[68];
    for (int k = 0; k < 68; k++) xf[k] = 0;
    double scale = 0;
    for (int k = 0; k < n; k++) scale += x[k] * (lambda * x[k] + bfull[k]);
    for (int h = 0; h < nf; h++) {
      Twh_t[h] = Twh[h]; aff_t[h][0] = aff[h][0]; aff_t[h][1] = aff[h][1];
      if (slot[h] < 0) continue;
      for (int k = 0; k < 8; k++) xf[h * 8 + k] = x[8 * slot[h] + k];
      Twh_t[h] = expSe3(&xf[h * 8]) * Twh[h];                          // VertexSE3PoseDSO::oplusImpl, dso_g2o_vertex.cpp:15-18
      aff_t[h][0] += xf[h * 8 + 6]; aff_t[h][1] += xf[h * 8 + 7];      // VertexPhotometricDSO::oplusImpl, :30-40
    }
    for (int k = 0; k < 4; k++) { xf[nf * 8 + k] = x[8 * nh + k]; cam_t[k] = cam[k] + xf[nf * 8 + k]; }   // VertexCamDSO::oplusImpl, :100-106
    SDSO_HIP(ctx, hipMemcpyAsync(d_x, xf, sizeof(double) * (nf * 8 + 4), hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    O.x = d_x;
    double sums[2];
    if ((rc = eval<2>(sums))) return rc;
    t->chi2 = sums[0];
    t->scale = scale + sums[1];
    return SDSO_OK;
  }
  void accept() {
    for (int h = 0; h < nf; h++) { Twh[h] = Twh_t[h]; aff[h][0] = aff_t[h][0]; aff[h][1] = aff_t[h][1]; }
    for (int k = 0; k < 4; k++) cam[k] = cam_t[k];
    cur ^= 1;
  }
  int evaluate(double* chi) {
    double sums[2];
    int rc = eval<1>(sums);
    if (rc) return rc;
    *chi = chi2 = sums[0];
    return SDSO_OK;
  }
};

static bool finite_se3(const sdso_se3_t& T) {
  for (int k = 0; k < 9; k++) if (!std::isfinite(T.R[k])) return false;
  for (int k = 0; k < 3; k++) if (!std::isfinite(T.t[k])) return false;
  return true;
}

// The refusals of the window optimiser, stated once for sdso_g2o_lba_optimize and sdso_g2o_lba_optimize_enqueue (g2o_lba_resident.hip),
// each before any device work.  `out` is checked where the entry point takes one (want_out).  Leaves the frames' level-0 images and the
// range of every host in the host-major order.
struct LbaCall {
  const float4* img[8];
  int hstart[9];
};
static int lba_validate(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, const sdso_g2o_lba_state_t* S,
                        const sdso_g2o_lba_result_t* out, bool want_out, LbaCall* call) {
  SDSO_REQUIRE(ctx, W && P && S && (out || !want_out), "null argument");
  const int nf = W->nf, nr = W->nr;
  SDSO_REQUIRE(ctx, nf >= 1 && nf <= 8, "nf must be 1..8");
  SDSO_REQUIRE(ctx, nr >= 0, "nr must not be negative");
  SDSO_REQUIRE(ctx, P->max_iterations >= 0, "max_iterations must not be negative");
  SDSO_REQUIRE(ctx, P->max_trials >= 1, "max_trials must be at least 1");
  SDSO_REQUIRE(ctx, std::isfinite(P->lambda_init) && std::isfinite(P->gain_threshold), "non-finite LM parameter");
  SDSO_REQUIRE(ctx, W->frame_slot && W->Ttw && W->target_aff && W->ab_exposure && W->host_b0 && W->frameEnergyTH, "null window array");
  SDSO_REQUIRE(ctx, S->Twh && S->host_aff, "null estimate array");
  if (nr > 0) {
    SDSO_REQUIRE(ctx, W->host && W->target && W->u && W->v && W->color && W->weights, "null window array");
    SDSO_REQUIRE(ctx, S->idepth, "null estimate array");
    if (want_out)
      SDSO_REQUIRE(ctx, out->state && out->energy && out->centerProjectedTo && out->edge_level && out->idepth_hessian && out->active, "null result array");
  }
  for (int f = 0; f < nf; f++) {
    auto ip = ctx->pyr.find(W->frame_slot[f]);
    SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), "unknown frame slot");
    SDSO_REQUIRE(ctx, ip->second.w[0] == W->w && ip->second.h[0] == W->h, "frame size mismatch");
    call->img[f] = ip->second.d[0];
    SDSO_REQUIRE(ctx, finite_se3(W->Ttw[f]) && finite_se3(S->Twh[f]), "non-finite pose");
    SDSO_REQUIRE(ctx, std::isfinite(W->target_aff[f].a) && std::isfinite(W->target_aff[f].b) && std::isfinite(S->host_aff[f].a) &&
                          std::isfinite(S->host_aff[f].b) && std::isfinite(W->ab_exposure[f]) && std::isfinite(W->host_b0[f]), "non-finite affine parameter");
  }
  for (int k = 0; k < 4; k++) SDSO_REQUIRE(ctx, std::isfinite(S->cam[k]), "non-finite camera parameter");
  for (int f = 0; f < 9; f++) call->hstart[f] = 0;
  for (int r = 0; r < nr; r++) {
    SDSO_REQUIRE(ctx, W->host[r] >= 0 && W->host[r] < nf && W->target[r] >= 0 && W->target[r] < nf, "host / target out of range");
    SDSO_REQUIRE(ctx, std::isfinite(W->u[r]) && std::isfinite(W->v[r]) && std::isfinite(S->idepth[r]), "non-finite point");
    call->hstart[W->host[r] + 1]++;
  }
  for (int f = 0; f < nf; f++) call->hstart[f + 1] += call->hstart[f];
  return SDSO_OK;
}

// host-major order: a stable counting sort, perm[sorted position] = the caller's index; the residual arrays in that order
struct LbaSorted {
  int *host, *target;
  float *u, *v, *color, *weights;
  double* idepth;
};
static void lba_sort_host_major(const sdso_g2o_lba_window_t* W, const double* idepth, const int* hstart, int* perm, const LbaSorted& o) {
  const int nf = W->nf, nr = W->nr;
  int fill[8];
  for (int f = 0; f < nf; f++) fill[f] = hstart[f];
  for (int r = 0; r < nr; r++) perm[fill[W->host[r]]++] = r;
  for (int i = 0; i < nr; i++) {
    const int r = perm[i];
    o.host[i] = W->host[r]; o.target[i] = W->target[r]; o.u[i] = W->u[r]; o.v[i] = W->v[r]; o.idepth[i] = idepth[r];
    std::memcpy(o.color + (size_t)i * 8, W->color + (size_t)r * 8, 32);
    std::memcpy(o.weights + (size_t)i * 8, W->weights + (size_t)r * 8, 32);
  }
}

// what a run without iterations leaves in `out` (and what every run starts from)
static void lba_result_reset(sdso_g2o_lba_result_t* out) {
  out->iterations = 0; out->stop = SDSO_G2O_LBA_STOP_ITERATIONS; out->n_active = 0; out->chi2_final = 0; out->rmse = 0;
  for (int i = 0; i < SDSO_G2O_LBA_MAX_RECORDED; i++) { out->trials[i] = 0; out->lambda[i] = 0; out->chi2[i] = 0; }
}

}  // namespace sdso

extern "C" int sdso_g2o_lba_optimize(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, sdso_g2o_lba_state_t* S,
                                     sdso_g2o_lba_result_t* out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  LbaCall call;
  SDSO_TRY(lba_validate(ctx, W, P, S, out, true, &call));
  const int nf = W->nf, nr = W->nr;
  LbaProblem Q;
  std::memset(&Q.O, 0, sizeof(Q.O));
  Q.ctx = ctx; Q.W = W; Q.nf = nf; Q.nr = nr;
  LbaDev& D = Q.O.L;
  D.nf = nf; D.nr = nr; D.w = W->w; D.h = W->h;
  for (int f = 0; f < nf; f++) {
    D.img[f] = call.img[f];
    Q.Twh[f] = se3_from_abi(S->Twh[f]);
    Q.aff[f][0] = S->host_aff[f].a; Q.aff[f][1] = S->host_aff[f].b;
    Q.n_active_host[f] = 0;
  }
  for (int k = 0; k < 4; k++) Q.cam[k] = S->cam[k];
  const int* hstart = call.hstart;
  lba_result_reset(out);
  if (nr == 0) return SDSO_OK;
  std::vector<int> perm(nr);
  std::vector<int> s_host(nr), s_tg(nr);
  std::vector<float> s_u(nr), s_v(nr), s_col((size_t)nr * 8), s_w((size_t)nr * 8);
  std::vector<double> s_id(nr);
  lba_sort_host_major(W, S->idepth, hstart, perm.data(), {s_host.data(), s_tg.data(), s_u.data(), s_v.data(), s_col.data(), s_w.data(), s_id.data()});
  // one device blob
  const size_t nn = (size_t)nf * nf;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t part_doubles = std::max<size_t>((size_t)nf * 2 * kLbaLinChunks * kLbaEnt, 2 * kLbaEvalBlocks);
  const size_t o_tab0 = take(sizeof(float) * nn * 14), o_tab1 = take(sizeof(float) * nn * 14), o_b0 = take(sizeof(double) * nf), o_eth = take(sizeof(float) * nf),
               o_hs = take(sizeof(int) * 9), o_cnt = take(sizeof(int) * 8), o_x = take(sizeof(double) * 68), o_part = take(sizeof(double) * part_doubles),
               o_sum = take(sizeof(double) * 8 * kLbaEnt), o_host = take(sizeof(int) * nr), o_tg = take(sizeof(int) * nr), o_u = take(sizeof(float) * nr),
               o_v = take(sizeof(float) * nr), o_id0 = take(sizeof(double) * nr), o_id1 = take(sizeof(double) * nr), o_col = take(sizeof(float) * 8 * nr),
               o_w = take(sizeof(float) * 8 * nr), o_rec = take(sizeof(double) * kLbaRec * (size_t)nr), o_act = take(nr), o_lv = take(nr), o_st = take(nr),
               o_en = take(sizeof(float) * 2 * nr), o_cpt = take(sizeof(float) * 3 * nr), o_ih = take(sizeof(float) * nr);
  int rc = ensure_scratch(ctx, off);
  if (rc) return rc;
  char* base = (char*)ctx->scratch;
#define UPL(o, src, bytes) SDSO_HIP(ctx, hipMemcpyAsync(base + (o), (src), (bytes), hipMemcpyHostToDevice, ctx->stream))
  UPL(o_b0, W->host_b0, sizeof(double) * nf); UPL(o_eth, W->frameEnergyTH, sizeof(float) * nf); UPL(o_hs, hstart, sizeof(int) * 9);
  UPL(o_host, s_host.data(), sizeof(int) * nr); UPL(o_tg, s_tg.data(), sizeof(int) * nr); UPL(o_u, s_u.data(), sizeof(float) * nr);
  UPL(o_v, s_v.data(), sizeof(float) * nr); UPL(o_id0, s_id.data(), sizeof(double) * nr); UPL(o_col, s_col.data(), sizeof(float) * 8 * nr);
  UPL(o_w, s_w.data(), sizeof(float) * 8 * nr);
#undef UPL
  SDSO_HIP(ctx, hipMemsetAsync(base + o_ih, 0, sizeof(float) * nr, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(base + o_rec, 0, sizeof(double) * kLbaRec * (size_t)nr, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(base + o_x, 0, sizeof(double) * 68, ctx->stream));
  D.host_b0 = (const double*)(base + o_b0); D.frameEnergyTH = (const float*)(base + o_eth);
  D.host = (const int*)(base + o_host); D.target = (const int*)(base + o_tg); D.u = (const float*)(base + o_u); D.v = (const float*)(base + o_v);
  D.color = (const float*)(base + o_col); D.weights = (const float*)(base + o_w);
  D.state = (uint8_t*)(base + o_st); D.energy = (float*)(base + o_en); D.cpt = (float*)(base + o_cpt); D.idepth_hessian = (float*)(base + o_ih);
  Q.O.hstart = (const int*)(base + o_hs); Q.O.active = (uint8_t*)(base + o_act); Q.O.level = (uint8_t*)(base + o_lv); Q.O.rec = (double*)(base + o_rec);
  Q.d_tab[0] = (float*)(base + o_tab0); Q.d_tab[1] = (float*)(base + o_tab1);
  Q.d_idepth[0] = (double*)(base + o_id0); Q.d_idepth[1] = (double*)(base + o_id1);
  Q.d_x = (double*)(base + o_x); Q.d_part = (double*)(base + o_part); Q.d_sum = (double*)(base + o_sum);
  Q.O.x = Q.d_x;

  // the build-time computeError (:539) fixes the active set (initializeOptimization, :587)
  double sums[2];
  if ((rc = Q.eval<0>(sums))) return rc;
  Q.chi2 = sums[0];
  hipLaunchKernelGGL(k_lba_opt_count, dim3(nf), dim3(256), 0, ctx->stream, Q.O.hstart, (const uint8_t*)Q.O.active, (int*)(base + o_cnt));
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipMemcpyAsync(Q.n_active_host, base + o_cnt, sizeof(int) * nf, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int n_active = 0;
  for (int f = 0; f < nf; f++) n_active += Q.n_active_host[f];
  g2o_lm::Result R;
  R.final_chi2 = Q.chi2;
  if (n_active > 0) {
    const g2o_lm::Params prm = {P->max_iterations, P->lambda_init, P->gain_threshold, P->max_trials};
    if ((rc = g2o_lm::run(Q, prm, Q.chi2, &R))) return rc;
  }
  // results: sorted order on the device, the caller's order on the host
  std::vector<uint8_t> r_st(nr), r_lv(nr), r_act(nr);
  std::vector<float> r_en((size_t)nr * 2), r_cpt((size_t)nr * 3), r_ih(nr);
#define DNL(dst, src, bytes) SDSO_HIP(ctx, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, ctx->stream))
  DNL(r_st.data(), base + o_st, nr); DNL(r_lv.data(), base + o_lv, nr); DNL(r_act.data(), base + o_act, nr);
  DNL(r_en.data(), base + o_en, sizeof(float) * 2 * nr); DNL(r_cpt.data(), base + o_cpt, sizeof(float) * 3 * nr); DNL(r_ih.data(), base + o_ih, sizeof(float) * nr);
  DNL(s_id.data(), Q.d_idepth[Q.cur], sizeof(double) * nr);
#undef DNL
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < nr; i++) {
    const int r = perm[i];
    out->state[r] = r_st[i]; out->edge_level[r] = r_lv[i]; out->active[r] = r_act[i]; out->idepth_hessian[r] = r_ih[i];
    out->energy[r * 2] = r_en[i * 2]; out->energy[r * 2 + 1] = r_en[i * 2 + 1];
    for (int k = 0; k < 3; k++) out->centerProjectedTo[r * 3 + k] = r_cpt[i * 3 + k];
    if (R.iterations > 0) S->idepth[r] = s_id[i];
  }
  if (R.iterations > 0) {
    for (int f = 0; f < nf; f++) {
      if (Q.n_active_host[f] == 0) continue;
      se3_to_abi(Q.Twh[f], S->Twh[f]);
      S->host_aff[f].a = Q.aff[f][0]; S->host_aff[f].b = Q.aff[f][1];
    }
    for (int k = 0; k < 4; k++) S->cam[k] = Q.cam[k];
  }
  out->iterations = R.iterations; out->stop = R.stop; out->n_active = n_active;
  for (int i = 0; i < SDSO_G2O_LBA_MAX_RECORDED; i++) { out->trials[i] = R.trials[i]; out->lambda[i] = R.lambda[i]; out->chi2[i] = R.chi2[i]; }
  out->chi2_final = R.final_chi2;
  out->rmse = sqrtf((float)(R.final_chi2 / (double)((size_t)8 * (size_t)nr)));   // :867: the quotient is a double, sqrtf takes it as a float
  return SDSO_OK;
}
