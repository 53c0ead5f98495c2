// The fused calcRes + calcGSSSE evaluation of the coarse tracker: its records, k_track_eval, k_track_finalize and the request table fill_eval (part of tracker.hip).
namespace sdso {

constexpr int TRK_BLOCK = 256;
constexpr int TRK_UNROLL = 4;  // template points per lane and loop trip (16 gathers in flight)
constexpr int TRK_NF = 48;  // float partials: 45 H + E + shiftT + shiftRT
constexpr int TRK_NI = 4;   // int partials: numTermsInE, numSaturated, numWarped, shiftNum

struct TrackProb {
  sdso_track_eval_t ev;
  const float4* pc;
  const float4* img;
  int n;
  int pad;
};

struct TrackOut {
  double H[64];
  double b[8];
  double res[6];
  int n_warped;
  int pad;
};

struct TrackBatch {
  int cap = 0, nprob = 0, gx = 0;
  DevBuf<TrackProb> d_probs;
  DevBuf<float> d_partF;
  DevBuf<int> d_partI;
  DevBuf<TrackOut> d_out;
  size_t part_cap = 0;
};

void release_track_batch(sdso_ctx* ctx) {
  delete ctx->tb;
  ctx->tb = nullptr;
}

}  // namespace sdso

#ifdef SDSO_LM_STAMPS   // diagnostic build (make EXTRA=-DSDSO_LM_STAMPS, tools/dbg_lm_stamps.py): shader-clock cycles of thread 0 per phase of k_track_lm
__shared__ unsigned long long lm_st_acc[16];
__shared__ unsigned long long lm_st_last;
#ifdef SDSO_LM_STAMPS_NOWAIT
#define LMS_WAIT
#else
#define LMS_WAIT asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
#define LMS(i) do { if (threadIdx.x == 0) { LMS_WAIT const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); lm_st_acc[i] += tn_ - lm_st_last; lm_st_last = tn_; } } while (0)
#else
#define LMS(i) do { } while (0)
#endif
// ------------------------------------------------------------------ kernels
// Per-lane sums of calcRes + calcGSSSE over the points first, first + stride, ... of one problem (TRK_UNROLL points per trip):
// the 45 upper-triangle products, E, the flow-indicator sums and the four counters.
struct TrackLaneSums {
  float acc[45];
  float E, sT, sRT;
  int nE, nSat, nWarp, nShift;
};
// PRE: the caller hands over the lane's TRK_UNROLL points of the FIRST trip (k_track_lm keeps them in registers while it stays on a
// level: the template does not move between evaluations); later trips (n > TRK_UNROLL * stride) load theirs.
template <bool MASK, bool PRE = false, int UNR = TRK_UNROLL>
__device__ __forceinline__ void track_accumulate(const sdso_track_eval_t& EV, const float4* __restrict__ pc, const float4* __restrict__ img, int n,
                                                 int first, int stride, uint8_t* __restrict__ mask, TrackLaneSums& Sout, const float4* qpre = nullptr) {
  TrackLaneSums S;   // a local, copied out at the end: accumulating through the reference cost 40 VGPRs (196 instead of 154: 2 waves per SIMD instead of 3)
  const int lvl = EV.lvl, wl = EV.w, hl = EV.h;
  const float fxl = EV.fx, fyl = EV.fy, cxl = EV.cx, cyl = EV.cy;
  const float affLL0 = EV.affLL[0], affLL1 = EV.affLL[1];
  const float b0 = EV.ref_b0, cutoffTH = EV.cutoffTH, huberTH = EV.huberTH;
  const float maxEnergy = 2 * huberTH * cutoffTH - huberTH * huberTH;
  float RKi[9], Ki[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; k++) { RKi[k] = EV.RKi[k]; Ki[k] = EV.Ki[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = EV.t[k];
  const float wlm3 = (float)(wl - 3), hlm3 = (float)(hl - 3);
  float* acc = S.acc;
#pragma unroll
  for (int k = 0; k < 45; k++) acc[k] = 0.f;
  float E = 0.f, sT = 0.f, sRT = 0.f;
  int nE = 0, nSat = 0, nWarp = 0, nShift = 0;

  // UNR template points per lane and trip, in three straight-line stages so that the memory system sees
  // all of a trip's requests at once: (1) the pc loads, (2) projection + bounds test + the 4 bilinear taps of every
  // point (an out-of-bounds point reads pixel (2,2) instead of branching around its loads), (3) residual, Huber,
  // the 45 products — in point order, so the per-lane sums are those of the one-point-per-trip loop.
  for (int i0 = first; i0 < n; i0 += UNR * stride) {
    float4 q[UNR];
#pragma unroll
    for (int s = 0; s < UNR; s++) {
      const int i = i0 + s * stride;
      if (PRE && i0 == first) q[s] = qpre[s]; else q[s] = pc[i < n ? i : i0];
    }
    LMS(1);
    float us[UNR], vs[UNR], nid[UNR];
    bool ok[UNR];
    float3 hits[UNR];
#pragma unroll
    for (int s = 0; s < UNR; s++) {
      const int i = i0 + s * stride;
      ok[s] = false; us[s] = 0.f; vs[s] = 0.f; nid[s] = 0.f; hits[s] = make_float3(0.f, 0.f, 0.f);
      if (i0 - first + s * stride >= n) continue;            // (uniform over the launch's threads: the whole slot is past the end — the coarse levels have fewer points than threads)
      const float x = q[s].x, y = q[s].y, id = q[s].z;
      float pt[3];
#pragma unroll
      for (int r = 0; r < 3; r++) pt[r] = ((RKi[r * 3 + 0] * x + RKi[r * 3 + 1] * y) + RKi[r * 3 + 2]) + t[r] * id;
      const float u = pt[0] / pt[2];
      const float v = pt[1] / pt[2];
      const float Ku = fxl * u + cxl;
      const float Kv = fyl * v + cyl;
      const float new_idepth = id / pt[2];
      us[s] = u; vs[s] = v; nid[s] = new_idepth;

      if (lvl == 0 && (i & 31) == 0 && i < n) {  // CoarseTracker.cpp:662-693 flow indicators
        float ptT[3], ptT2[3], pt3[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const float kp = (Ki[r * 3 + 0] * x + Ki[r * 3 + 1] * y) + Ki[r * 3 + 2];
          const float rp = (RKi[r * 3 + 0] * x + RKi[r * 3 + 1] * y) + RKi[r * 3 + 2];
          ptT[r] = kp + t[r] * id;
          ptT2[r] = kp - t[r] * id;
          pt3[r] = rp - t[r] * id;
        }
        const float KuT = fxl * (ptT[0] / ptT[2]) + cxl, KvT = fyl * (ptT[1] / ptT[2]) + cyl;
        const float KuT2 = fxl * (ptT2[0] / ptT2[2]) + cxl, KvT2 = fyl * (ptT2[1] / ptT2[2]) + cyl;
        const float Ku3 = fxl * (pt3[0] / pt3[2]) + cxl, Kv3 = fyl * (pt3[1] / pt3[2]) + cyl;
        sT += (KuT - x) * (KuT - x) + (KvT - y) * (KvT - y);
        sT += (KuT2 - x) * (KuT2 - x) + (KvT2 - y) * (KvT2 - y);
        sRT += (Ku - x) * (Ku - x) + (Kv - y) * (Kv - y);
        sRT += (Ku3 - x) * (Ku3 - x) + (Kv3 - y) * (Kv3 - y);
        nShift += 2;
      }
      ok[s] = i < n && Ku > 2 && Kv > 2 && Ku < wlm3 && Kv < hlm3 && new_idepth > 0;  // :696
      hits[s] = interp33(img, ok[s] ? Ku : 2.5f, ok[s] ? Kv : 2.5f, wl);
    }
    LMS(2);
#pragma unroll
    for (int s = 0; s < UNR; s++) {
      const int i = i0 + s * stride;
      if (i0 - first + s * stride >= n) continue;
      const float u = us[s], v = vs[s], new_idepth = nid[s], refColor = q[s].w;
      const float3 hit = hits[s];
      bool inl = false;
      if (ok[s] && isfinite(hit.x)) {
        const float residual = hit.x - (affLL0 * refColor + affLL1);
        const float ar = fabsf(residual);
        const float hw = ar < huberTH ? 1.f : huberTH / ar;
        nE++;
        if (ar > cutoffTH) {
          E += maxEnergy;
          nSat++;
        } else {
          E += hw * residual * residual * (2 - hw);
          nWarp++;
          inl = true;
          // calcGSSSE rows (:555-577), same nesting as the SSE expressions
          const float dx = hit.y * fxl;
          const float dy = hit.z * fyl;
          float J[9];
          J[0] = new_idepth * dx;
          J[1] = new_idepth * dy;
          J[2] = 0.0f - new_idepth * (u * dx + v * dy);
          J[3] = 0.0f - ((u * v) * dx + dy * (1.0f + v * v));
          J[4] = (u * v) * dy + dx * (1.0f + u * u);
          J[5] = u * dy - v * dx;
          J[6] = affLL0 * (b0 - refColor);
          J[7] = -1.0f;
          J[8] = residual;
          int k = 0;
#pragma unroll
          for (int r = 0; r < 9; r++) {
            const float Jw = J[r] * hw;
#pragma unroll
            for (int c = r; c < 9; c++) { acc[k] = __builtin_fmaf(Jw, J[c], acc[k]); k++; }
          }
        }
      }
      if (MASK && i < n) mask[i] = inl ? 1 : 0;
    }
  }
  S.E = E; S.sT = sT; S.sRT = sRT; S.nE = nE; S.nSat = nSat; S.nWarp = nWarp; S.nShift = nShift;
  Sout = S;
}

template <bool MASK>
__global__ __launch_bounds__(TRK_BLOCK) void k_track_eval(const TrackProb* __restrict__ probs, int nprob, int gx,
                                                          float* __restrict__ partF, int* __restrict__ partI,
                                                          uint8_t* __restrict__ mask) {
  // XCD-aware mapping: linear workgroup id L runs on XCD (L % 8); give every chunk of problem p
  // the same residue so one L2 serves the problem's image.  Speed only; any placement is correct.
  const int L = blockIdx.x;
  const int xcd = L & 7;
  const int j = L >> 3;
  const int p = (j / gx) * 8 + xcd;
  const int bx = j % gx;
  if (p >= nprob) return;
  const TrackProb& P = probs[p];
  const int n = P.n;
  if (bx > 0 && bx * TRK_BLOCK >= n) return;   // no points for this workgroup (k_track_finalize skips its partial)
  TrackLaneSums S;
  track_accumulate<MASK>(P.ev, P.pc, P.img, n, bx * TRK_BLOCK + threadIdx.x, gx * TRK_BLOCK, mask, S);
  float* acc = S.acc;
  const float E = S.E, sT = S.sT, sRT = S.sRT;
  const int nE = S.nE, nSat = S.nSat, nWarp = S.nWarp, nShift = S.nShift;

  // ---- workgroup reduction: 64-lane butterfly, then 4 waves through LDS
  __shared__ float sF[TRK_BLOCK / 64][TRK_NF];
  __shared__ int sI[TRK_BLOCK / 64][TRK_NI];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    float v48[TRK_NF];
#pragma unroll
    for (int k = 0; k < 45; k++) v48[k] = acc[k];
    v48[45] = E; v48[46] = sT; v48[47] = sRT;
    wave_reduce_rows<TRK_NF>(v48, [&](int k, float s) { sF[wv][k] = s; });
  }
  {
    int i0 = nE, i1 = nSat, i2 = nWarp, i3 = nShift;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      i0 += __shfl_xor(i0, o, 64); i1 += __shfl_xor(i1, o, 64); i2 += __shfl_xor(i2, o, 64); i3 += __shfl_xor(i3, o, 64);
    }
    if (lane == 0) { sI[wv][0] = i0; sI[wv][1] = i1; sI[wv][2] = i2; sI[wv][3] = i3; }
  }
  __syncthreads();
  const size_t rec = (size_t)p * gx + bx;
  if (threadIdx.x < TRK_NF) {
    float s = sF[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < TRK_BLOCK / 64; w++) s += sF[w][threadIdx.x];
    partF[rec * TRK_NF + threadIdx.x] = s;
  } else if (threadIdx.x < TRK_NF + TRK_NI) {
    const int k = threadIdx.x - TRK_NF;
    int s = sI[0][k];
#pragma unroll
    for (int w = 1; w < TRK_BLOCK / 64; w++) s += sI[w][k];
    partI[rec * TRK_NI + k] = s;
  }
}

// calcRes' Vec6 (:783-789) from an evaluation's sums, for k_track_finalize and for wave 0 of k_track_lm
__device__ __forceinline__ void track_res6(float E, float sT, float sRT, int nE, int nSat, int nShift, double* res) {
  res[0] = (double)E;
  res[1] = (double)nE;
  res[2] = (double)sT / ((double)(float)nShift + 0.1);
  res[3] = 0;
  res[4] = (double)sRT / ((double)(float)nShift + 0.1);
  res[5] = (double)((float)nSat / (float)nE);
}

// Fold the per-workgroup partials of each problem (fixed order) and finish like calcGSSSE :580-595
// and calcRes :783-789.
__global__ __launch_bounds__(64) void k_track_finalize(const TrackProb* __restrict__ probs, const float* __restrict__ partF,
                                                       const int* __restrict__ partI, int gx, TrackOut* __restrict__ out) {
  const int p = blockIdx.x;
  const int nb = min(gx, max(1, (probs[p].n + TRK_BLOCK - 1) / TRK_BLOCK));   // workgroups that had points
  __shared__ float F[TRK_NF];
  __shared__ int I[TRK_NI];
  const int tid = threadIdx.x;
  if (tid < TRK_NF) {
    float s = 0.f;
    for (int b = 0; b < nb; b++) s += partF[((size_t)p * gx + b) * TRK_NF + tid];
    F[tid] = s;
  } else if (tid < TRK_NF + TRK_NI) {
    int s = 0;
    for (int b = 0; b < nb; b++) s += partI[((size_t)p * gx + b) * TRK_NI + tid - TRK_NF];
    I[tid - TRK_NF] = s;
  }
  __syncthreads();
  const int nE = I[0], nSat = I[1], nWarp = I[2], nShift = I[3];
  const int npad = (nWarp + 3) & ~3;  // buf_warped_n with its zero padding (:763-775)
  TrackOut& O = out[p];
  const double SC[8] = {SCALE_XI_ROT, SCALE_XI_ROT, SCALE_XI_ROT, SCALE_XI_TRANS, SCALE_XI_TRANS, SCALE_XI_TRANS, SCALE_A, SCALE_B};
  const float inv_n = 1.0f / npad;
  // upper-triangle index of (r,c), r<=c, 9 columns
  for (int e = tid; e < 72; e += 64) {
    const int r = e / 9, c = e % 9;  // r in 0..7, c in 0..8
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const int idx = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
    double v = npad > 0 ? (double)F[idx] * (double)inv_n : 0.0;
    if (c < 8) { v *= SC[c]; v *= SC[r]; O.H[r * 8 + c] = v; }
    else { v *= SC[r]; O.b[r] = v; }
  }
  if (tid == 0) {
    track_res6(F[45], F[46], F[47], nE, nSat, nShift, O.res);
    O.n_warped = npad;
  }
}

// ------------------------------------------------------------------ host side
// The request of one evaluation, given Ki = K[lvl]^-1 (k_track_lm keeps it per level; fill_eval computes it).
SDSO_HD static void fill_eval_ki(const sdso_track_params_t& p, int lvl, const float* Ki, const Se3& T, const sdso_aff_t& aff, float cutoff, sdso_track_eval_t& ev) {
  ev.lvl = lvl; ev.w = p.w[lvl]; ev.h = p.h[lvl];
  ev.fx = p.fx[lvl]; ev.fy = p.fy[lvl]; ev.cx = p.cx[lvl]; ev.cy = p.cy[lvl];
  for (int i = 0; i < 9; i++) ev.Ki[i] = Ki[i];
  float Rf[9];
  for (int i = 0; i < 9; i++) Rf[i] = (float)T.R[i];
  mul3f(Rf, ev.Ki, ev.RKi);                          // :617
  for (int i = 0; i < 3; i++) ev.t[i] = (float)T.t[i];
  double a2[2];
  affFromTo(p.ref_exposure, p.new_exposure, p.ref_aff_g2l.a, p.ref_aff_g2l.b, aff.a, aff.b, a2);
  ev.affLL[0] = (float)a2[0]; ev.affLL[1] = (float)a2[1];
  ev.ref_b0 = (float)p.ref_aff_g2l.b;
  ev.cutoffTH = cutoff;
  ev.huberTH = p.huberTH;
}
SDSO_HD static void fill_eval(const sdso_track_params_t& p, int lvl, const Se3& T, const sdso_aff_t& aff, float cutoff, sdso_track_eval_t& ev) {
  const float K[9] = {p.fx[lvl], 0, p.cx[lvl], 0, p.fy[lvl], p.cy[lvl], 0, 0, 1};
  float Ki[9];
  inv3f(K, Ki);                                      // CoarseTracker.cpp:129-130
  fill_eval_ki(p, lvl, Ki, T, aff, cutoff, ev);
}
