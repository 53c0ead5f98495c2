// The device-resident immature points of a ctx (sdso_imm_*): FullSystem::makeNewTraces, traceNewCoarseKey / traceNewCoarseNonKey and
// STEP 5 of activatePointsMT on arrays that never leave the device.  Included at the end of stereo.hip: it reuses TraceDev,
// k_immature_init, trace_on_point, k_trace_stereo_blk (launch_trace_stereo) and the TraceBatch helpers of the matching batches.
//
// Reference (paths under /root/reference):
//   src/FullSystem/FullSystem.cpp:1600-1629   makeNewTraces
//   src/FullSystem/FullSystem.cpp:632-781     traceNewCoarseNonKey, traceNewCoarseKey
//   src/FullSystem/FullSystem.cpp:948-957     activatePointsMT STEP 5
//   src/FullSystem/ImmaturePoint.cpp:33-88    the two constructors
//
// Layout: one blob of kImmFloats * cap floats and cap status bytes per host, structure of arrays with stride cap (color, weights, gradH
// and lastTraceUV keep the point-major inner layout of TraceDev, so a host's blob binds to a TraceDev without a copy).  Every host has a
// second blob of the same size: sdso_imm_remove gathers into it and the two swap.
namespace sdso {

constexpr int kImmFloats = 30;
enum { IMM_U = 0, IMM_V = 1, IMM_TYPE = 2, IMM_IMIN = 3, IMM_IMAX = 4, IMM_QUAL = 5, IMM_COLOR = 6, IMM_WEIGHTS = 14, IMM_GRADH = 22, IMM_ETH = 26,
       IMM_UV = 27, IMM_INTERVAL = 29 };   // offsets in units of cap floats
enum { IMM_C_FWD_GOOD = 6, IMM_C_STEREO_OUTLIER = 7, IMM_C_UPDATED = 8, IMM_C_UNREADABLE = 9 };

struct ImmHostDev { float* f; uint8_t* st; int n, cap; };
struct ImmHost {
  int w = 0, h = 0, cap = 0;
  int n = -1;                       // -1: the count of the add that made this host has not been read yet (h_n is valid after ev)
  float* f[2] = {nullptr, nullptr}; // [0] current, [1] the target of the next removal gather
  uint8_t* st[2] = {nullptr, nullptr};
  int* d_n = nullptr;
  int* h_n = nullptr;               // pinned
  hipEvent_t ev = nullptr;
};
struct ImmState {
  std::map<int, ImmHost> hosts;
  TraceBatch fwd, back;             // the stereo chain of the non-key trace, over the concatenated points of the named hosts
  int* d_counts = nullptr;          // SDSO_IMM_NCOUNTS
  int* h_counts = nullptr;          // pinned
  StageBuf stage;                   // selection maps and removal orders on their way to the device
};
static ImmState& imm_state(sdso_ctx* ctx) { if (!ctx->imm) ctx->imm = new ImmState(); return *ctx->imm; }
static void imm_free_host(ImmHost& H) {
  for (int k = 0; k < 2; k++) { if (H.f[k]) hipFree(H.f[k]); if (H.st[k]) hipFree(H.st[k]); }
  if (H.d_n) hipFree(H.d_n);
  if (H.h_n) hipHostFree(H.h_n);
  if (H.ev) hipEventDestroy(H.ev);
  H = ImmHost();
}
static int imm_alloc_host(sdso_ctx* ctx, ImmHost& H) {   // the caller frees what was allocated when this fails
  const size_t C = (size_t)H.cap;
  for (int k = 0; k < 2; k++) {
    SDSO_HIP(ctx, hipMalloc(&H.f[k], sizeof(float) * kImmFloats * C));
    SDSO_HIP(ctx, hipMalloc(&H.st[k], C));
  }
  SDSO_HIP(ctx, hipMalloc(&H.d_n, sizeof(int)));
  SDSO_HIP(ctx, hipHostMalloc((void**)&H.h_n, sizeof(int)));
  SDSO_HIP(ctx, hipEventCreateWithFlags(&H.ev, hipEventDisableTiming));
  return SDSO_OK;
}
void release_immature(sdso_ctx* ctx) {
  ImmState* S = ctx->imm;
  if (!S) return;
  for (auto& kv : S->hosts) imm_free_host(kv.second);
  trace_free(S->fwd); trace_free(S->back);
  if (S->d_counts) hipFree(S->d_counts);
  if (S->h_counts) hipHostFree(S->h_counts);
  stage_free(S->stage);
  delete S;
  ctx->imm = nullptr;
}
// the host-side count of a host: waits for the add that made it, not for the stream
static int imm_resolve(sdso_ctx* ctx, ImmHost& H) {
  if (H.n >= 0) return SDSO_OK;
  SDSO_HIP(ctx, hipEventSynchronize(H.ev));
  H.n = *H.h_n;
  return SDSO_OK;
}

// a host's blob as the TraceDev of traceOn: u_stereo / v_stereo = u / v, idepth_min_stereo / idepth_max_stereo = idepth_min / idepth_max
__host__ __device__ inline void imm_bind(TraceDev& T, float* f, uint8_t* st, int cap, int n) {
  const size_t N = (size_t)cap;
  T.n = n;
  T.u_stereo = f + IMM_U * N; T.v_stereo = f + IMM_V * N; T.idepth_min = f + IMM_IMIN * N;
  T.idepth_min_stereo = f + IMM_IMIN * N; T.idepth_max_stereo = f + IMM_IMAX * N; T.idepth_stereo = nullptr;
  T.quality = f + IMM_QUAL * N; T.color = f + IMM_COLOR * N; T.weights = f + IMM_WEIGHTS * N; T.gradH = f + IMM_GRADH * N;
  T.energyTH = f + IMM_ETH * N; T.lastTraceUV = f + IMM_UV * N; T.lastTracePixelInterval = f + IMM_INTERVAL * N;
  T.lastTraceStatus = st; T.status = nullptr; T.skip = nullptr;
}

// ---- ordered compaction: items [0, N) in segments of L, one workgroup per segment.  segcount -> scan -> segwrite gives every item that
// satisfies the predicate its rank among them, in item order (raster order for the map: L = w, one segment per row).
struct ImmMapPred {   // the loop bounds and the test of FullSystem.cpp:1611-1614
  const float* map; int w, h;
  __device__ bool operator()(int idx) const {
    const int x = idx % w, y = idx / w;
    return x >= 3 && x < w - 4 && y >= 3 && y < h - 4 && map[idx] != 0;
  }
};
struct ImmMapEmit {   // candidate (x, y, map[i]) of :1616
  const float* map; int w, cap; float *u, *v, *type;
  __device__ void operator()(int idx, int pos) const {
    if (pos >= cap) return;
    u[pos] = (float)(idx % w); v[pos] = (float)(idx / w); type[pos] = map[idx];
  }
};
struct ImmKeepPred {  // :1619: the constructor left a finite energyTH
  const int* ncand; const float* energyTH;
  __device__ bool operator()(int idx) const { return idx < *ncand && isfinite(energyTH[idx]); }
};
struct ImmStoreEmit { // the members of a new ImmaturePoint (ImmaturePoint.cpp:33-62) at its place in the host's arrays
  const float *u, *v, *type, *color, *weights, *gradH, *energyTH;
  float* f; uint8_t* st; int cap;
  __device__ void operator()(int idx, int pos) const {
    if (pos >= cap) return;
    const size_t N = (size_t)cap;
    f[IMM_U * N + pos] = u[idx]; f[IMM_V * N + pos] = v[idx]; f[IMM_TYPE * N + pos] = type[idx];
    f[IMM_IMIN * N + pos] = 0.f; f[IMM_IMAX * N + pos] = NAN; f[IMM_QUAL * N + pos] = 10000.f;
    for (int k = 0; k < 8; k++) { f[IMM_COLOR * N + (size_t)pos * 8 + k] = color[(size_t)idx * 8 + k]; f[IMM_WEIGHTS * N + (size_t)pos * 8 + k] = weights[(size_t)idx * 8 + k]; }
    for (int k = 0; k < 4; k++) f[IMM_GRADH * N + (size_t)pos * 4 + k] = gradH[(size_t)idx * 4 + k];
    f[IMM_ETH * N + pos] = energyTH[idx];
    f[IMM_UV * N + (size_t)pos * 2] = 0.f; f[IMM_UV * N + (size_t)pos * 2 + 1] = 0.f; f[IMM_INTERVAL * N + pos] = 0.f;
    st[pos] = IPS_UNINITIALIZED;
  }
};

}  // namespace sdso

template <class Pred>
__global__ __launch_bounds__(256) void k_imm_segcount(Pred pred, int N, int L, int* __restrict__ cnt) {
  __shared__ int s[4];
  const int base = blockIdx.x * L;
  int c = 0;
  for (int x0 = 0; x0 < L; x0 += 256) {
    const int x = x0 + threadIdx.x, idx = base + x;
    const bool on = x < L && idx < N && pred(idx);
    c += __popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}
// exclusive scan of cnt[0 .. nseg) in place, one workgroup; *total = the sum
__global__ __launch_bounds__(256) void k_imm_scan(int* __restrict__ cnt, int nseg, int* __restrict__ total) {
  __shared__ int s[256];
  const int t = threadIdx.x, per = (nseg + 255) / 256;
  const int b = t * per, e = min(nseg, b + per);
  int sum = 0;
  for (int k = b; k < e; k++) sum += cnt[k];
  s[t] = sum;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 256; k++) { const int c = s[k]; s[k] = run; run += c; }
    *total = run;
  }
  __syncthreads();
  int run = s[t];
  for (int k = b; k < e; k++) { const int c = cnt[k]; cnt[k] = run; run += c; }
}
// ordered writes inside a segment: rank = segment offset + items before this chunk + waves before this one + lanes before this one
template <class Pred, class Emit>
__global__ __launch_bounds__(256) void k_imm_segwrite(Pred pred, Emit emit, int N, int L, const int* __restrict__ off) {
  __shared__ int s[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * L;
  int run = off[blockIdx.x];
  for (int x0 = 0; x0 < L; x0 += 256) {
    const int x = x0 + threadIdx.x, idx = base + x;
    const bool on = x < L && idx < N && pred(idx);
    const unsigned long long m = __ballot(on);
    if (lane == 0) s[wv] = __popcll(m);
    __syncthreads();
    int pos = run;
    for (int k = 0; k < wv; k++) pos += s[k];
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (on) emit(idx, pos);
    run += s[0] + s[1] + s[2] + s[3];
    __syncthreads();
  }
}

namespace sdso {
// the named hosts of one sdso_imm_trace call, as kernel arguments (a few hundred bytes: nothing is copied to the device per call)
struct ImmTraceArgs {
  int nh, ntot;
  int off[SDSO_IMM_MAX_HOSTS + 1];   // first flat index of every host; flat index j = off[g] + i
  ImmHostDev H[SDSO_IMM_MAX_HOSTS];
  sdso_imm_geom_t G[SDSO_IMM_MAX_HOSTS];
};
struct ImmCalib { float Ki[9]; };
__device__ __forceinline__ int imm_host_of(const ImmTraceArgs& A, int j) {
  int g = 0;
  while (g + 1 < A.nh && j >= A.off[g + 1]) g++;
  return g;
}
}  // namespace sdso

// ImmaturePoint::traceOn for every point of the named hosts, in place: one wave per point, the body of k_trace_on
__global__ __launch_bounds__(256) void k_imm_trace_on(ImmTraceArgs A, TraceDev base) {
  const int wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wv;
  if (j >= A.ntot) return;
  __shared__ float s_err[4][128];
  const int g = imm_host_of(A, j);
  TraceDev T = base;
  imm_bind(T, A.H[g].f, A.H[g].st, A.H[g].cap, A.H[g].n);
  trace_on_point(T, j - A.off[g], s_err[wv], [&] {
    sdso_trace_geom_t G;
    for (int k = 0; k < 9; k++) G.KRKi[k] = A.G[g].KRKi[k];
    for (int k = 0; k < 3; k++) G.Kt[k] = A.G[g].Kt[k];
    G.aff[0] = A.G[g].aff[0]; G.aff[1] = A.G[g].aff[1];
    return G;
  });
}

// a fresh point parked on a harmless pixel (the constructor kernel reads valid memory, the trace kernel skips it)
__device__ __forceinline__ void imm_fresh_point(const TraceDev& T, int j, float u, float v, float idepth_min, float imin_stereo, float imax_stereo) {
  T.u_stereo[j] = u; T.v_stereo[j] = v;
  T.idepth_min[j] = idepth_min;
  T.idepth_min_stereo[j] = imin_stereo; T.idepth_max_stereo[j] = imax_stereo;
  T.idepth_stereo[j] = 0.f; T.quality[j] = 10000.f; T.lastTraceStatus[j] = IPS_UNINITIALIZED;
  T.lastTraceUV[2 * j] = 0.f; T.lastTraceUV[2 * j + 1] = 0.f; T.lastTracePixelInterval[j] = 0.f;
}
// counts[k] += the lanes of the wave with `on` (one atomic per wave; every lane of the wave calls)
__device__ __forceinline__ void imm_count(int* __restrict__ counts, int k, bool on) {
  const int c = __popcll(__ballot(on));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[k], c);
}
__device__ __forceinline__ bool imm_readable(float u, float v, int w, int h) { return u >= 2 && v >= 2 && u < w - 3 && v < h - 3; }

// FullSystem.cpp:671-686: selects the points whose traceOn returned GOOD (skip = 0), projects their interval into the new frame and makes
// the forward points at lastTraceUV
__global__ __launch_bounds__(256) void k_imm_stereo_prepare(ImmTraceArgs A, int w, int h, TraceDev F, uint8_t* __restrict__ skip, float* __restrict__ pmin,
                                                            float* __restrict__ pmax, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < A.ntot;
  const int g = in ? imm_host_of(A, j) : 0, i = in ? j - A.off[g] : 0;
  const float* f = A.H[g].f;
  const size_t N = (size_t)A.H[g].cap;
  bool run = false, unreadable = false;
  float fu = 8.f, fv = 8.f, pm = 0.f, pM = NAN;
  if (in && A.H[g].st[i] == IPS_GOOD) {
    const float tu = f[IMM_UV * N + (size_t)i * 2], tv = f[IMM_UV * N + (size_t)i * 2 + 1];
    if (imm_readable(tu, tv, w, h)) {
      run = true; fu = tu; fv = tv;
      const float u = f[IMM_U * N + i], v = f[IMM_V * N + i], imin = f[IMM_IMIN * N + i], imax = f[IMM_IMAX * N + i];
      const float* KRKi = A.G[g].KRKi;
      const float Kt2 = A.G[g].Kt[2];
      pm = 1.0f / (((KRKi[6] * (u / imin) + KRKi[7] * (v / imin)) + KRKi[8] * (1.0f / imin)) + Kt2);
      pM = 1.0f / (((KRKi[6] * (u / imax) + KRKi[7] * (v / imax)) + KRKi[8] * (1.0f / imax)) + Kt2);
    } else unreadable = true;
  }
  imm_count(counts, IMM_C_UNREADABLE, unreadable);
  if (!in) return;
  skip[j] = run ? 0 : 1;
  pmin[j] = pm; pmax[j] = pM;
  imm_fresh_point(F, j, fu, fv, pm, pm, pM);   // :681-686: idepth_min and idepth_min_stereo are both the projection
}
// :691-697: the back points at the forward trace's lastTraceUV, with the projected interval again
__global__ __launch_bounds__(256) void k_imm_back_points(int n, int w, int h, TraceDev F, TraceDev Bk, const uint8_t* __restrict__ skipF, uint8_t* __restrict__ skipB,
                                                         const float* __restrict__ pmin, const float* __restrict__ pmax, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool good = false, run = false;
  if (j < n) {
    float bu = 8.f, bv = 8.f;
    good = !skipF[j] && F.lastTraceStatus[j] == IPS_GOOD;
    if (good) {
      const float tu = F.lastTraceUV[2 * j], tv = F.lastTraceUV[2 * j + 1];
      if (imm_readable(tu, tv, w, h)) { run = true; bu = tu; bv = tv; }
    }
    skipB[j] = run ? 0 : 1;
    imm_fresh_point(Bk, j, bu, bv, 0.f, run ? pmin[j] : 0.f, run ? pmax[j] : NAN);
  }
  imm_count(counts, IMM_C_FWD_GOOD, good);
  imm_count(counts, IMM_C_UNREADABLE, good && !run);
}
// :703-720: the accept rule and the back-projection of the stereo-refined interval into the host
__global__ __launch_bounds__(256) void k_imm_accept(ImmTraceArgs A, ImmCalib C, TraceDev F, TraceDev Bk, const uint8_t* __restrict__ skipB, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool outlier = false, updated = false;
  if (j < A.ntot && !skipB[j]) {
    const int g = imm_host_of(A, j), i = j - A.off[g];
    const float us = F.u_stereo[j], vs = F.v_stereo[j];
    const float u_stereo_delta = fabsf(us - Bk.lastTraceUV[2 * j]);
    const float disparity = us - F.lastTraceUV[2 * j];
    if (u_stereo_delta > 1 && disparity < 10) {
      A.H[g].st[i] = IPS_OUTLIER;
      outlier = true;
    } else {
      const float* Ki = C.Ki;
      const float* KRi = A.G[g].KRi;
      const float* t = A.G[g].t;
      const float q0 = (Ki[0] * us + Ki[1] * vs) + Ki[2] * 1.0f, q1 = (Ki[3] * us + Ki[4] * vs) + Ki[5] * 1.0f, q2 = (Ki[6] * us + Ki[7] * vs) + Ki[8] * 1.0f;
      float out[2];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float s = k == 0 ? F.idepth_min_stereo[j] : F.idepth_max_stereo[j];
        const float p0 = q0 / s - t[0], p1 = q1 / s - t[1], p2 = q2 / s - t[2];
        out[k] = 1.0f / ((KRi[6] * p0 + KRi[7] * p1) + KRi[8] * p2);
      }
      const size_t N = (size_t)A.H[g].cap;
      A.H[g].f[IMM_IMIN * N + i] = out[0];
      A.H[g].f[IMM_IMAX * N + i] = out[1];
      updated = true;
    }
  }
  imm_count(counts, IMM_C_STEREO_OUTLIER, outlier);
  imm_count(counts, IMM_C_UPDATED, updated);
}
__global__ __launch_bounds__(256) void k_imm_hist(ImmTraceArgs A, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  int st = 255;
  if (j < A.ntot) { const int g = imm_host_of(A, j); st = A.H[g].st[j - A.off[g]]; }
  for (int s = 0; s < 6; s++) {
    const int c = __popcll(__ballot(st == s));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[s], c);
  }
}
// STEP 5 on the device: entry j of the new arrays is entry src[j] of the old ones, every member
__global__ __launch_bounds__(256) void k_imm_gather(int n_new, const int* __restrict__ src, const float* __restrict__ f, const uint8_t* __restrict__ st, float* __restrict__ fo,
                                                    uint8_t* __restrict__ sto, int cap) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = q / (kImmFloats + 1), c = q % (kImmFloats + 1);
  if (j >= n_new) return;
  const int i = src[j];
  if (c == kImmFloats) { sto[j] = st[i]; return; }
  // member and width of float c of a point: {u v type imin imax quality} 1, color 8, weights 8, gradH 4, energyTH 1, UV 2, interval 1
  int o, wd;
  if (c < 6) { o = c; wd = 1; }
  else if (c < 14) { o = IMM_COLOR; wd = 8; }
  else if (c < 22) { o = IMM_WEIGHTS; wd = 8; }
  else if (c < 26) { o = IMM_GRADH; wd = 4; }
  else if (c < 27) { o = IMM_ETH; wd = 1; }
  else if (c < 29) { o = IMM_UV; wd = 2; }
  else { o = IMM_INTERVAL; wd = 1; }
  const size_t N = (size_t)cap, k = (size_t)(c - o);
  fo[o * N + (size_t)j * wd + k] = f[o * N + (size_t)i * wd + k];
}

// ------------------------------------------------------------------ API
extern "C" int sdso_imm_add_frame(sdso_ctx* ctx, int host_id, int frame_slot, const float* selection_map, int* n_out) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  auto ip = ctx->pyr.find(frame_slot);
  SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), "unknown frame slot");
  const int w = ip->second.w[0], h = ip->second.h[0];
  SDSO_REQUIRE(ctx, w >= 16 && h >= 16, "image too small for the pattern");
  ImmState& S = imm_state(ctx);
  SDSO_REQUIRE(ctx, S.hosts.find(host_id) == S.hosts.end(), "the host already has immature points");
  const size_t npx = (size_t)w * h;
  // the number of candidates bounds every buffer: counted here for a host map, the selector's own count for its map
  int ncand = 0;
  const float* d_map = nullptr;
  if (selection_map) {
    for (int y = 3; y < h - 4; y++)
      for (int x = 3; x < w - 4; x++) ncand += selection_map[x + (size_t)y * w] != 0;
  } else if (!selector_final_map(ctx, frame_slot, w, h, &d_map, &ncand))
    return sdso::fail(ctx, SDSO_ERR_STATE, "no map of sdso_pixel_select on this frame slot");
  const int cap = std::max(ncand, 1), nseg2 = (cap + 255) / 256;
  // scratch: [map] | candidates u v type color weights gradH energyTH (24 floats) | row offsets | segment offsets | candidate count
  const size_t bytes = (selection_map ? sizeof(float) * npx : 0) + sizeof(float) * 24 * (size_t)cap + sizeof(int) * ((size_t)h + nseg2 + 4);
  int rc = ensure_scratch(ctx, bytes);
  if (rc) return rc;
  float* q = (float*)ctx->scratch;
  if (selection_map) {
    char* stage = nullptr;
    rc = stage_reserve(ctx, S.stage, sizeof(float) * npx, &stage);
    if (rc) return rc;
    std::copy(selection_map, selection_map + npx, (float*)stage);
    SDSO_HIP(ctx, hipMemcpyAsync(q, stage, sizeof(float) * npx, hipMemcpyHostToDevice, ctx->stream));
    rc = stage_commit(ctx, S.stage);
    if (rc) return rc;
    d_map = q; q += npx;
  }
  const size_t C = (size_t)cap;
  float *cu = q, *cv = q + C, *ct = q + 2 * C, *cc = q + 3 * C, *cw = q + 11 * C, *cg = q + 19 * C, *ce = q + 23 * C;
  int* d_row = (int*)(q + 24 * C);
  int* d_seg = d_row + h;
  int* d_ncand = d_seg + nseg2;

  ImmHost H;
  H.w = w; H.h = h; H.cap = cap;
  rc = imm_alloc_host(ctx, H);
  if (rc) { imm_free_host(H); return rc; }

  auto enqueue = [&]() -> int {
    const int one = 0x41000000;   // 8.0f: candidates past the count (the selector's bound) sit on a harmless pixel for the constructor kernel
    SDSO_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)cu, one, 2 * C, ctx->stream));
    const ImmMapPred mp{d_map, w, h};
    const ImmMapEmit me{d_map, w, cap, cu, cv, ct};
    launch_timed(ctx, "k_imm_map_count", 2, k_imm_segcount<ImmMapPred>, dim3(h), dim3(256), mp, (int)npx, w, d_row);
    launch_timed(ctx, "k_imm_scan", 2, k_imm_scan, dim3(1), dim3(256), d_row, h, d_ncand);
    launch_timed(ctx, "k_imm_map_write", 2, (k_imm_segwrite<ImmMapPred, ImmMapEmit>), dim3(h), dim3(256), mp, me, (int)npx, w, (const int*)d_row);
    launch_timed(ctx, "k_immature_init", 2, k_immature_init, dim3(nseg2), dim3(256), (const float4*)ip->second.d[0], w, cap, (const float*)cu, (const float*)cv, cc, cw, cg, ce);
    const ImmKeepPred kp{d_ncand, ce};
    const ImmStoreEmit ke{cu, cv, ct, cc, cw, cg, ce, H.f[0], H.st[0], cap};
    launch_timed(ctx, "k_imm_keep_count", 2, k_imm_segcount<ImmKeepPred>, dim3(nseg2), dim3(256), kp, cap, 256, d_seg);
    launch_timed(ctx, "k_imm_scan", 2, k_imm_scan, dim3(1), dim3(256), d_seg, nseg2, H.d_n);
    launch_timed(ctx, "k_imm_keep_write", 2, (k_imm_segwrite<ImmKeepPred, ImmStoreEmit>), dim3(nseg2), dim3(256), kp, ke, cap, 256, (const int*)d_seg);
    SDSO_HIP(ctx, hipGetLastError());
    SDSO_HIP(ctx, hipMemcpyAsync(H.h_n, H.d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipEventRecord(H.ev, ctx->stream));
    return SDSO_OK;
  };
  rc = enqueue();
  if (rc) { hipStreamSynchronize(ctx->stream); imm_free_host(H); return rc; }   // the host is not in the set yet: nothing else owns its buffers
  ImmHost& R = S.hosts[host_id];
  R = H;
  if (n_out) {
    rc = imm_resolve(ctx, R);
    if (rc) return rc;
    *n_out = R.n;
  }
  return SDSO_OK;
}

extern "C" int sdso_imm_trace(sdso_ctx* ctx, int frame_slot, int right_slot, int ngeom, const sdso_imm_geom_t* geom, const float K[4], const float Ki[9],
                              float baseline, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const bool nonkey = right_slot >= 0;
  SDSO_REQUIRE(ctx, ngeom >= 0 && ngeom <= SDSO_IMM_MAX_HOSTS && (ngeom == 0 || geom), "0 <= ngeom <= SDSO_IMM_MAX_HOSTS geometries");
  SDSO_REQUIRE(ctx, !nonkey || (K && Ki), "the non-key trace needs K and Ki");
  auto il = ctx->pyr.find(frame_slot);
  SDSO_REQUIRE(ctx, il != ctx->pyr.end(), "unknown frame slot");
  const int w = il->second.w[0], h = il->second.h[0];
  auto ir = ctx->pyr.end();
  if (nonkey) {
    ir = ctx->pyr.find(right_slot);
    SDSO_REQUIRE(ctx, ir != ctx->pyr.end(), "unknown right frame slot");
    SDSO_REQUIRE(ctx, ir->second.w[0] == w && ir->second.h[0] == h, "the two frames differ in size");
  }
  ImmState& S = imm_state(ctx);
  ImmHost* hosts[SDSO_IMM_MAX_HOSTS];
  for (int g = 0; g < ngeom; g++) {
    auto it = S.hosts.find(geom[g].host_id);
    SDSO_REQUIRE(ctx, it != S.hosts.end(), "unknown host_id");
    for (int k = 0; k < g; k++) SDSO_REQUIRE(ctx, geom[k].host_id != geom[g].host_id, "host_id named twice");
    SDSO_REQUIRE(ctx, it->second.w == w && it->second.h == h, "the frame differs in size from the host's");
    hosts[g] = &it->second;
  }
  ImmTraceArgs A;
  A.nh = ngeom; A.off[0] = 0;
  for (int g = 0; g < ngeom; g++) {
    int rc = imm_resolve(ctx, *hosts[g]);
    if (rc) return rc;
    A.H[g] = ImmHostDev{hosts[g]->f[0], hosts[g]->st[0], hosts[g]->n, hosts[g]->cap};
    A.G[g] = geom[g];
    A.off[g + 1] = A.off[g] + hosts[g]->n;
  }
  for (int g = ngeom; g < SDSO_IMM_MAX_HOSTS; g++) { A.H[g] = ImmHostDev{nullptr, nullptr, 0, 0}; A.G[g] = sdso_imm_geom_t(); A.off[g + 1] = A.off[ngeom]; }
  const int n = A.ntot = A.off[ngeom];
  if (counts) for (int k = 0; k < SDSO_IMM_NCOUNTS; k++) counts[k] = 0;
  if (n == 0) return SDSO_OK;
  if (!S.d_counts) {
    SDSO_HIP(ctx, hipMalloc(&S.d_counts, sizeof(int) * SDSO_IMM_NCOUNTS));
    SDSO_HIP(ctx, hipHostMalloc((void**)&S.h_counts, sizeof(int) * SDSO_IMM_NCOUNTS));
  }
  int rc = ensure_plane0(ctx, il->second);
  if (rc) return rc;
  if (nonkey) {
    rc = ensure_plane0(ctx, ir->second);
    if (rc) return rc;
    rc = trace_reserve(ctx, S.fwd, n);
    if (rc) return rc;
    rc = trace_reserve(ctx, S.back, n);
    if (rc) return rc;
  }
  SDSO_HIP(ctx, hipMemsetAsync(S.d_counts, 0, sizeof(int) * SDSO_IMM_NCOUNTS, ctx->stream));
  TraceDev base = TraceDev();
  base.w = w; base.h = h; base.mode_right = 1; base.fx = 1; base.fy = 1; base.cx = 0; base.cy = 0; base.baseline = 0;
  base.img = il->second.d[0]; base.plane = il->second.plane0;
  launch_timed(ctx, "k_imm_trace_on", 1, k_imm_trace_on, dim3((n + 3) / 4), dim3(256), A, base);
  if (nonkey) {
    trace_bind(S.fwd, n); trace_bind(S.back, n);
    TraceDev& F = S.fwd.T;
    TraceDev& Bk = S.back.T;
    auto cam = [&](TraceDev& T, const PyramidDev& P, int mode_right) {
      T.w = w; T.h = h; T.mode_right = mode_right; T.img = P.d[0]; T.plane = P.plane0;
      T.fx = K[0]; T.fy = K[1]; T.cx = K[2]; T.cy = K[3]; T.baseline = baseline;
    };
    cam(F, ir->second, 1);     // forward: points of the new left frame searched in the right one
    cam(Bk, il->second, 0);    // back: points of the right frame searched in the left one
    uint8_t* skipF = S.fwd.bytes + 2 * (size_t)S.fwd.n;
    uint8_t* skipB = S.back.bytes + 2 * (size_t)S.back.n;
    float* pmin = S.fwd.blob + 32 * (size_t)S.fwd.n;
    float* pmax = S.fwd.blob + 33 * (size_t)S.fwd.n;
    ImmCalib C;
    for (int k = 0; k < 9; k++) C.Ki[k] = Ki[k];
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_stereo_prepare", 2, k_imm_stereo_prepare, g1, b1, A, w, h, F, skipF, pmin, pmax, S.d_counts);
    launch_timed(ctx, "k_immature_init", 2, k_immature_init, g1, b1, (const float4*)il->second.d[0], w, n, (const float*)F.u_stereo, (const float*)F.v_stereo,
                 (float*)F.color, (float*)F.weights, (float*)F.gradH, (float*)F.energyTH);
    TraceDev Ff = F;
    Ff.skip = skipF;
    launch_trace_stereo(ctx, Ff, true);
    launch_timed(ctx, "k_imm_back_points", 2, k_imm_back_points, g1, b1, n, w, h, F, Bk, (const uint8_t*)skipF, skipB, (const float*)pmin, (const float*)pmax, S.d_counts);
    launch_timed(ctx, "k_immature_init", 2, k_immature_init, g1, b1, (const float4*)ir->second.d[0], w, n, (const float*)Bk.u_stereo, (const float*)Bk.v_stereo,
                 (float*)Bk.color, (float*)Bk.weights, (float*)Bk.gradH, (float*)Bk.energyTH);
    TraceDev Bb = Bk;
    Bb.skip = skipB;
    launch_trace_stereo(ctx, Bb, true);
    launch_timed(ctx, "k_imm_accept", 2, k_imm_accept, g1, b1, A, C, F, Bk, (const uint8_t*)skipB, S.d_counts);
  }
  SDSO_HIP(ctx, hipGetLastError());
  if (counts) {
    launch_timed(ctx, "k_imm_hist", 2, k_imm_hist, dim3((n + 255) / 256), dim3(256), A, S.d_counts);
    SDSO_HIP(ctx, hipGetLastError());
    SDSO_HIP(ctx, hipMemcpyAsync(S.h_counts, S.d_counts, sizeof(int) * SDSO_IMM_NCOUNTS, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < SDSO_IMM_NCOUNTS; k++) counts[k] = S.h_counts[k];
  }
  return SDSO_OK;
}

extern "C" int sdso_imm_count(sdso_ctx* ctx, int host_id, int* n) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, n, "null argument");
  *n = 0;
  if (!ctx->imm) return SDSO_OK;
  auto it = ctx->imm->hosts.find(host_id);
  if (it == ctx->imm->hosts.end()) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  int rc = imm_resolve(ctx, it->second);
  if (rc) return rc;
  *n = it->second.n;
  return SDSO_OK;
}

extern "C" int sdso_imm_get(sdso_ctx* ctx, int host_id, sdso_trace_points_t* out, float* my_type) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, out, "null argument");
  ImmState& S = imm_state(ctx);
  auto it = S.hosts.find(host_id);
  SDSO_REQUIRE(ctx, it != S.hosts.end(), "unknown host_id");
  ImmHost& H = it->second;
  int rc = imm_resolve(ctx, H);
  if (rc) return rc;
  const int n = out->n = H.n;
  if (n == 0) return SDSO_OK;
  const float* f = H.f[0];
  const size_t N = (size_t)H.cap;
#define DN(dst, off, cnt) if (dst) SDSO_HIP(ctx, hipMemcpyAsync((dst), f + (off) * N, sizeof(float) * (size_t)(cnt), hipMemcpyDeviceToHost, ctx->stream))
  DN(out->u_stereo, IMM_U, n); DN(out->v_stereo, IMM_V, n); DN(my_type, IMM_TYPE, n);
  DN(out->idepth_min_stereo, IMM_IMIN, n); DN(out->idepth_max_stereo, IMM_IMAX, n); DN(out->quality, IMM_QUAL, n);
  DN(out->color, IMM_COLOR, 8 * n); DN(out->weights, IMM_WEIGHTS, 8 * n); DN(out->gradH, IMM_GRADH, 4 * n); DN(out->energyTH, IMM_ETH, n);
  DN(out->lastTraceUV, IMM_UV, 2 * n); DN(out->lastTracePixelInterval, IMM_INTERVAL, n);
#undef DN
  if (out->lastTraceStatus) SDSO_HIP(ctx, hipMemcpyAsync(out->lastTraceStatus, H.st[0], n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

extern "C" int sdso_imm_remove_order(int n, const uint8_t* flags, int* n_out, int* src) {
  if (n < 0 || !n_out || (n && (!flags || !src))) return SDSO_ERR_ARG;
  // the vector holds old indices; a flagged entry stands for the reference's null pointer
  for (int i = 0; i < n; i++) src[i] = i;
  int size = n;
  for (int i = 0; i < size; i++)
    if (flags[src[i]]) { src[i] = src[size - 1]; size--; i--; }
  *n_out = size;
  return SDSO_OK;
}

extern "C" int sdso_imm_remove(sdso_ctx* ctx, int host_id, int n, const uint8_t* flags) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  ImmState& S = imm_state(ctx);
  auto it = S.hosts.find(host_id);
  SDSO_REQUIRE(ctx, it != S.hosts.end(), "unknown host_id");
  ImmHost& H = it->second;
  int rc = imm_resolve(ctx, H);
  if (rc) return rc;
  SDSO_REQUIRE(ctx, n == H.n && (n == 0 || flags), "n differs from the host's count");
  if (n == 0) return SDSO_OK;
  char* stage = nullptr;
  rc = stage_reserve(ctx, S.stage, sizeof(int) * (size_t)n, &stage);
  if (rc) return rc;
  int n_new = 0;
  rc = sdso_imm_remove_order(n, flags, &n_new, (int*)stage);
  if (rc) return sdso::fail(ctx, rc, "sdso_imm_remove_order");
  if (n_new == n) return SDSO_OK;   // nothing flagged: the order does not change
  H.n = n_new;
  if (n_new == 0) return SDSO_OK;
  rc = ensure_scratch(ctx, sizeof(int) * (size_t)n_new);
  if (rc) return rc;
  int* d_src = (int*)ctx->scratch;
  SDSO_HIP(ctx, hipMemcpyAsync(d_src, stage, sizeof(int) * (size_t)n_new, hipMemcpyHostToDevice, ctx->stream));
  rc = stage_commit(ctx, S.stage);
  if (rc) return rc;
  const int threads = n_new * (kImmFloats + 1);
  launch_timed(ctx, "k_imm_gather", 2, k_imm_gather, dim3((threads + 255) / 256), dim3(256), n_new, (const int*)d_src, (const float*)H.f[0], (const uint8_t*)H.st[0], H.f[1],
               H.st[1], H.cap);
  SDSO_HIP(ctx, hipGetLastError());
  std::swap(H.f[0], H.f[1]);
  std::swap(H.st[0], H.st[1]);
  return SDSO_OK;
}

extern "C" int sdso_imm_release_host(sdso_ctx* ctx, int host_id) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->imm) return SDSO_OK;
  auto it = ctx->imm->hosts.find(host_id);
  if (it == ctx->imm->hosts.end()) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // launches that read the host's arrays may still be in flight
  imm_free_host(it->second);
  ctx->imm->hosts.erase(it);
  return SDSO_OK;
}
