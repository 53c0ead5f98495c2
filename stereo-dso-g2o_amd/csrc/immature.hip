// The device-resident immature points of a ctx (sdso_imm_*): FullSystem::makeNewTraces, traceNewCoarseKey / traceNewCoarseNonKey and
// STEP 5 of activatePointsMT on arrays that never leave the device.  Included at the end of stereo.hip: the searches are stereo.hip's
// trace_on_point and k_trace_stereo_blk (the pieces of trace_dev.h), the stereo chain of the non-key trace is launched with
// trace_pair_bind / launch_fresh_trace around this file's own prepare / back / accept kernels, and new points are written by fresh_point.
//
// Reference (paths under /root/reference):
//   src/FullSystem/FullSystem.cpp:1600-1629   makeNewTraces
//   src/FullSystem/FullSystem.cpp:632-781     traceNewCoarseNonKey, traceNewCoarseKey
//   src/FullSystem/FullSystem.cpp:948-957     activatePointsMT STEP 5
//   src/FullSystem/FullSystem.cpp:837-957     activatePointsMT STEP 2-5 in place (sdso_imm_activate, at the end of this file)
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
  StageBuf stage;                   // selection maps, removal orders and sdso_imm_activate's tables on their way to the device
  // the results of the latest sdso_imm_activate: header | decisions | records (pinned), for sdso_imm_activate_fetch
  char* h_act = nullptr;
  size_t h_act_cap = 0;
  bool act_valid = false;
  int act_nf = 0, act_ntot = 0, act_nsel = 0;
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
  if (S->h_act) hipHostFree(S->h_act);
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
template <class Args>
__device__ __forceinline__ int imm_host_of(const Args& A, int j) {
  int g = 0;
  while (g + 1 < A.nh && j >= A.off[g + 1]) g++;
  return g;
}
}  // namespace sdso

// ImmaturePoint::traceOn for every point of the named hosts, in place: one wave per point, the body of k_trace_on
__global__ __launch_bounds__(256) void k_imm_trace_on(ImmTraceArgs A, TraceDev base) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j);
  TraceDev T = base;
  imm_bind(T, A.H[g].f, A.H[g].st, A.H[g].cap, A.H[g].n);
  trace_on_point(T, j - A.off[g], [&] {
    sdso_trace_geom_t G;
    for (int k = 0; k < 9; k++) G.KRKi[k] = A.G[g].KRKi[k];
    for (int k = 0; k < 3; k++) G.Kt[k] = A.G[g].Kt[k];
    G.aff[0] = A.G[g].aff[0]; G.aff[1] = A.G[g].aff[1];
    return G;
  });
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
  float fu = 8.f, fv = 8.f, pm = 0.f, pM = NAN;   // a point that takes no trace is parked on a harmless pixel: the constructor kernel reads valid memory
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
  fresh_point(F, j, fu, fv, pm, pm, pM);   // :681-686: idepth_min and idepth_min_stereo are both the projection
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
    fresh_point(Bk, j, bu, bv, 0.f, run ? pmin[j] : 0.f, run ? pmax[j] : NAN);
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
// STEP 5 on the device: float c (c == kImmFloats: the status byte) of entry j of the new arrays is that of entry i of the old ones
__device__ __forceinline__ void imm_gather_one(int j, int i, int c, const float* __restrict__ f, const uint8_t* __restrict__ st, float* __restrict__ fo,
                                               uint8_t* __restrict__ sto, int cap) {
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
// entry j of the new arrays is entry src[j] of the old ones, every member
__global__ __launch_bounds__(256) void k_imm_gather(int n_new, const int* __restrict__ src, const float* __restrict__ f, const uint8_t* __restrict__ st, float* __restrict__ fo,
                                                    uint8_t* __restrict__ sto, int cap) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = q / (kImmFloats + 1), c = q % (kImmFloats + 1);
  if (j >= n_new) return;
  imm_gather_one(j, src[j], c, f, st, fo, sto, cap);
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
    rc = trace_pair_bind(ctx, S.fwd, S.back, n, il->second, ir->second, K, baseline, 1, 0);
    if (rc) return rc;
  }
  SDSO_HIP(ctx, hipMemsetAsync(S.d_counts, 0, sizeof(int) * SDSO_IMM_NCOUNTS, ctx->stream));
  TraceDev base = TraceDev();
  base.w = w; base.h = h; base.mode_right = 1; base.fx = 1; base.fy = 1; base.cx = 0; base.cy = 0; base.baseline = 0;
  base.img = il->second.d[0]; base.plane = il->second.plane0;
  launch_timed(ctx, "k_imm_trace_on", 1, k_imm_trace_on, dim3((n + 3) / 4), dim3(256), A, base);
  if (nonkey) {
    const TraceDev& F = S.fwd.T;     // forward: points of the new left frame searched in the right one
    const TraceDev& Bk = S.back.T;   // back: points of the right frame searched in the left one
    uint8_t* skipF = S.fwd.bytes + 2 * (size_t)S.fwd.n;
    uint8_t* skipB = S.back.bytes + 2 * (size_t)S.back.n;
    float* pmin = S.fwd.blob + 32 * (size_t)S.fwd.n;
    float* pmax = S.fwd.blob + 33 * (size_t)S.fwd.n;
    ImmCalib C;
    for (int k = 0; k < 9; k++) C.Ki[k] = Ki[k];
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_stereo_prepare", 2, k_imm_stereo_prepare, g1, b1, A, w, h, F, skipF, pmin, pmax, S.d_counts);
    launch_fresh_trace(ctx, F, il->second, skipF);
    launch_timed(ctx, "k_imm_back_points", 2, k_imm_back_points, g1, b1, n, w, h, F, Bk, (const uint8_t*)skipF, skipB, (const float*)pmin, (const float*)pmax, S.d_counts);
    launch_fresh_trace(ctx, Bk, ir->second, skipB);
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

extern "C" int sdso_imm_put_host(sdso_ctx* ctx, int host_id, int w, int h, const sdso_trace_points_t* P, const float* my_type) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, P && P->n >= 0, "null argument");
  SDSO_REQUIRE(ctx, w >= 16 && h >= 16, "image too small for the pattern");
  const int n = P->n;
  SDSO_REQUIRE(ctx, n == 0 || (my_type && P->u_stereo && P->v_stereo && P->idepth_min_stereo && P->idepth_max_stereo && P->quality && P->color && P->weights &&
                               P->gradH && P->energyTH && P->lastTraceStatus && P->lastTraceUV && P->lastTracePixelInterval), "null point array");
  ImmState& S = imm_state(ctx);
  SDSO_REQUIRE(ctx, S.hosts.find(host_id) == S.hosts.end(), "the host already has immature points");
  ImmHost H;
  H.w = w; H.h = h; H.cap = std::max(n, 1); H.n = n;
  int rc = imm_alloc_host(ctx, H);
  if (rc) { imm_free_host(H); return rc; }
  auto copy = [&]() -> int {
    const size_t N = (size_t)H.cap;
    float* f = H.f[0];
#define UP(src, off, cnt) SDSO_HIP(ctx, hipMemcpyAsync(f + (off) * N, (src), sizeof(float) * (size_t)(cnt), hipMemcpyHostToDevice, ctx->stream))
    UP(P->u_stereo, IMM_U, n); UP(P->v_stereo, IMM_V, n); UP(my_type, IMM_TYPE, n);
    UP(P->idepth_min_stereo, IMM_IMIN, n); UP(P->idepth_max_stereo, IMM_IMAX, n); UP(P->quality, IMM_QUAL, n);
    UP(P->color, IMM_COLOR, 8 * n); UP(P->weights, IMM_WEIGHTS, 8 * n); UP(P->gradH, IMM_GRADH, 4 * n); UP(P->energyTH, IMM_ETH, n);
    UP(P->lastTraceUV, IMM_UV, 2 * n); UP(P->lastTracePixelInterval, IMM_INTERVAL, n);
#undef UP
    SDSO_HIP(ctx, hipMemcpyAsync(H.st[0], P->lastTraceStatus, n, hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the arrays are the caller's again when the call returns
    return SDSO_OK;
  };
  if (n) {
    rc = copy();
    if (rc) { hipStreamSynchronize(ctx->stream); imm_free_host(H); return rc; }
  }
  S.hosts[host_id] = H;
  return SDSO_OK;
}

// ------------------------------------------------------------------ activatePointsMT STEP 2-5 on the set (FullSystem.cpp:837-957)
// sdso_imm_activate enqueues, without a host round trip in between:
//   k_imm_act_classify   the gates of STEP 2 per candidate, read from the groups' blobs (dm_classify, shared with k_select_classify)
//   k_distmap_select     the order-dependent rest of STEP 2 (distmap.hip, unchanged)
//   segcount/scan/write  the SELECTed candidates in order = toOptimize
//   k_imm_activate       optimizeImmaturePoint per entry of that list, one wave per point (activate_point, shared with
//                        k_activate_points); writes the entry's record and the STEP 4 flag of its candidate
//   k_imm_act_prefix     per group: exclusive prefix of the flags
//   k_imm_act_back/_src  the removal order of STEP 5 in closed form (below), then k_imm_act_gather into the groups' second blobs
namespace sdso {

struct ImmActArgs {
  int nf, nh, ntot;                    // nh = nf - 1 walked frames
  int off[SDSO_IMM_MAX_HOSTS + 1];     // first candidate of every walked frame; candidate j = off[g] + i
  ImmHostDev H[SDSO_IMM_MAX_HOSTS];    // the group of frame g (n = 0 without one)
  sdso_distmap_geom_t G[SDSO_IMM_MAX_HOSTS];
  uint8_t flagged[SDSO_IMM_MAX_HOSTS];
};
struct ImmActOut { float* f[SDSO_IMM_MAX_HOSTS]; uint8_t* st[SDSO_IMM_MAX_HOSTS]; };
// one entry of toOptimize as sdso_imm_activate_fetch hands it out
struct ImmActRec {
  int frame, index;
  int8_t status; uint8_t lastTraceStatus; uint8_t pad[2];
  float idepth;
  uint8_t res_state[8];
  float u, v, my_type, idepth_min, idepth_max, energyTH;
  float color[8], weights[8];
};
static_assert(sizeof(ImmActRec) == 112, "records are copied as 16-byte aligned blocks");
// header of the result blob: ints
enum { ACT_H_DELETE = 0, ACT_H_NSEL = 1, ACT_H_NLIST = 2, ACT_H_STATUS = 3 /* -1, 0, 1 */, ACT_H_FLAGGED = 6 /* per walked frame */, ACT_H_INTS = 16 };

// one candidate of the resident set, for dm_classify
struct ImmCand {
  const float* f; const uint8_t* st; size_t N; int i;
  const sdso_distmap_geom_t& G; bool flag;
  __device__ uint8_t status() const { return st[i]; }
  __device__ float imax() const { return f[IMM_IMAX * N + i]; }
  __device__ float imin() const { return f[IMM_IMIN * N + i]; }
  __device__ float interval() const { return f[IMM_INTERVAL * N + i]; }
  __device__ float quality() const { return f[IMM_QUAL * N + i]; }
  __device__ bool flagged() const { return flag; }
  __device__ const sdso_distmap_geom_t& geom() const { return G; }
  __device__ float u() const { return f[IMM_U * N + i]; }
  __device__ float v() const { return f[IMM_V * N + i]; }
};
struct ImmSelPred {   // decided SELECT by k_distmap_select
  const uint8_t* dec;
  __device__ bool operator()(int idx) const { return dec[idx] == DM_SELECT; }
};
struct ImmListEmit {  // toOptimize.push_back (:894)
  int* list;
  __device__ void operator()(int idx, int pos) const { list[pos] = idx; }
};

}  // namespace sdso

__global__ __launch_bounds__(256) void k_imm_act_classify(ImmActArgs A, float minActDist, float minTraceQuality, int w1, int h1, uint8_t* __restrict__ dec,
                                                          uint8_t* __restrict__ flag, int* __restrict__ iu, int* __restrict__ iv, float* __restrict__ frac,
                                                          float* __restrict__ thr, int* __restrict__ hdr) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool del = false;
  if (j < A.ntot) {
    const int g = imm_host_of(A, j), i = j - A.off[g];
    const size_t N = (size_t)A.H[g].cap;
    int pu = 0, pv = 0;
    float fr = 0.f;
    const uint8_t d = dm_classify(ImmCand{A.H[g].f, A.H[g].st, N, i, A.G[g], A.flagged[g] != 0}, minTraceQuality, w1, h1, pu, pv, fr);
    del = d == DM_DELETE;
    dec[j] = d;
    flag[j] = del ? 1 : 0;                                                             // STEP 4: `delete ph; host->immaturePoints[i] = 0`
    iu[j] = pu; iv[j] = pv; frac[j] = fr;
    thr[j] = minActDist * A.H[g].f[IMM_TYPE * N + i];                                  // :892
  }
  imm_count(hdr, ACT_H_DELETE, del);
}

// STEP 3 + the STEP 4 rule over toOptimize, one wave per entry.  The list's length is on the device: the grid covers the candidates, the
// waves past the list leave at once
__global__ __launch_bounds__(256) void k_imm_activate(ImmActArgs A, ActDev D, const int* __restrict__ list, const int* __restrict__ n_list, ImmActRec* rec,
                                                      uint8_t* flag, int* hdr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.x * 4 + wv;
  if (p >= *n_list) return;
  {
    const int j = list[p];
    const int g = imm_host_of(A, j), i = j - A.off[g];
    const float* f = A.H[g].f;
    const size_t N = (size_t)A.H[g].cap;
    const int idx = lane & 7;
    const float u = f[IMM_U * N + i], v = f[IMM_V * N + i], imin = f[IMM_IMIN * N + i], imax = f[IMM_IMAX * N + i], eth = f[IMM_ETH * N + i];
    const float color = f[IMM_COLOR * N + (size_t)i * 8 + idx], wgt = f[IMM_WEIGHTS * N + (size_t)i * 8 + idx];
    ImmActRec& R = rec[p];
    activate_point(D, lane, g, u, v, color, wgt, eth, imin, imax, &R.status, &R.idepth, R.res_state);
    if (lane < 8) { R.color[lane] = color; R.weights[lane] = wgt; }
    if (lane == 0) {
      for (int k = D.nf; k < 8; k++) R.res_state[k] = 255;
      const uint8_t lts = A.H[g].st[i];
      R.frame = g; R.index = i; R.lastTraceStatus = lts; R.pad[0] = 0; R.pad[1] = 0;
      R.u = u; R.v = v; R.my_type = f[IMM_TYPE * N + i]; R.idepth_min = imin; R.idepth_max = imax; R.energyTH = eth;
      const int s = R.status;                                                          // this lane's own store
      if (s != 0 || lts == IPS_OOB) flag[j] = 1;                                       // :923-941
      atomicAdd(&hdr[ACT_H_STATUS + s + 1], 1);                                        // one lane of the wave
    }
  }
}

// pref[j] = the number of flagged entries before entry i of its group; hdr[ACT_H_FLAGGED + g] = the group's total.  One workgroup per group.
__global__ __launch_bounds__(256) void k_imm_act_prefix(ImmActArgs A, const uint8_t* __restrict__ flag, int* __restrict__ pref, int* __restrict__ hdr) {
  __shared__ int s[256];
  const int g = blockIdx.x, t = threadIdx.x;
  const int n = A.H[g].n, base = A.off[g];
  const int per = (n + 255) / 256;
  const int b = min(n, t * per), e = min(n, b + per);
  int sum = 0;
  for (int k = b; k < e; k++) sum += flag[base + k];
  s[t] = sum;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 256; k++) { const int c = s[k]; s[k] = run; run += c; }
    hdr[ACT_H_FLAGGED + g] = run;
  }
  __syncthreads();
  int run = s[t];
  for (int k = b; k < e; k++) { pref[base + k] = run; run += flag[base + k]; }
}
// The loop of STEP 5 in closed form.  With m survivors of n entries: survivors at indices < m stay; the flagged indices < m, ascending,
// receive the survivors at indices >= m, descending (every `= back(); pop_back()` hands the last live entry to the first hole; flagged
// entries at the back are popped on the way).  back[k] = the k-th survivor from the back, for the survivors at indices >= m.
__global__ __launch_bounds__(256) void k_imm_act_back(ImmActArgs A, const uint8_t* __restrict__ flag, const int* __restrict__ pref, const int* __restrict__ hdr,
                                                      int* __restrict__ back) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j), i = j - A.off[g];
  const int n = A.H[g].n, nflag = hdr[ACT_H_FLAGGED + g], m = n - nflag;
  if (flag[j] || i < m) return;
  const int k = (n - 1 - i) - (nflag - pref[j]);          // survivors behind entry i
  back[A.off[g] + k] = i;
}
// src[j] (i < m) = the old index of the entry that ends at index i: itself, or for the k-th hole the k-th survivor from the back
__global__ __launch_bounds__(256) void k_imm_act_src(ImmActArgs A, const uint8_t* __restrict__ flag, const int* __restrict__ pref, const int* __restrict__ hdr,
                                                     const int* __restrict__ back, int* __restrict__ src) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j), i = j - A.off[g];
  const int m = A.H[g].n - hdr[ACT_H_FLAGGED + g];
  if (i >= m) return;
  src[j] = flag[j] ? back[A.off[g] + pref[j]] : i;
}
// k_imm_gather for every walked group that loses an entry, in one launch, with the new counts read on the device
__global__ __launch_bounds__(256) void k_imm_act_gather(ImmActArgs A, ImmActOut O, const int* __restrict__ hdr, const int* __restrict__ src) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = q / (kImmFloats + 1), c = q % (kImmFloats + 1);
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j), i = j - A.off[g];
  const int nflag = hdr[ACT_H_FLAGGED + g];
  if (nflag == 0 || i >= A.H[g].n - nflag) return;
  imm_gather_one(i, src[j], c, A.H[g].f, A.H[g].st, O.f[g], O.st[g], A.H[g].cap);
}

extern "C" int sdso_imm_activate(sdso_ctx* ctx, const sdso_imm_activate_t* P, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  int w1 = 0, h1 = 0;
  if (!distmap_dims(ctx, &w1, &h1)) return sdso::fail(ctx, SDSO_ERR_STATE, "no distance map yet (sdso_distmap_make)");
  SDSO_REQUIRE(ctx, P, "null argument");
  const int nf = P->nf, nh = nf - 1;
  SDSO_REQUIRE(ctx, nf >= 2 && nf <= SDSO_IMM_MAX_HOSTS, "2 <= nf <= 8 keyframes");
  SDSO_REQUIRE(ctx, P->host_id && P->frame_slot && P->host_flagged && P->geom && P->pair_R && P->pair_t && P->pair_aff, "null array");
  SDSO_REQUIRE(ctx, (P->w >> 1) == w1 && (P->h >> 1) == h1, "image size differs from the distance map's");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  ImmState& S = imm_state(ctx);
  const float4* imgs[SDSO_IMM_MAX_HOSTS] = {nullptr};
  ImmHost* hosts[SDSO_IMM_MAX_HOSTS] = {nullptr};
  for (int f = 0; f < nf; f++) {
    for (int k = 0; k < f; k++) SDSO_REQUIRE(ctx, P->host_id[k] != P->host_id[f], "host_id named twice");
    auto ip = ctx->pyr.find(P->frame_slot[f]);
    SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), "unknown frame slot");
    SDSO_REQUIRE(ctx, ip->second.w[0] == P->w && ip->second.h[0] == P->h, "pyramid size differs from w/h");
    imgs[f] = ip->second.d[0];
    auto it = S.hosts.find(P->host_id[f]);
    if (it == S.hosts.end()) continue;
    SDSO_REQUIRE(ctx, it->second.w == P->w && it->second.h == P->h, "the group's frame differs in size from w/h");
    hosts[f] = &it->second;
  }
  ImmActArgs A;
  ImmActOut O;
  A.nf = nf; A.nh = nh; A.off[0] = 0;
  for (int g = 0; g < SDSO_IMM_MAX_HOSTS; g++) {
    A.H[g] = ImmHostDev{nullptr, nullptr, 0, 0}; A.G[g] = sdso_distmap_geom_t(); A.flagged[g] = 0; O.f[g] = nullptr; O.st[g] = nullptr;
    if (g < nh && hosts[g]) {
      int rc = imm_resolve(ctx, *hosts[g]);
      if (rc) return rc;
      A.H[g] = ImmHostDev{hosts[g]->f[0], hosts[g]->st[0], hosts[g]->n, hosts[g]->cap};
      O.f[g] = hosts[g]->f[1]; O.st[g] = hosts[g]->st[1];
    }
    if (g < nh) { A.G[g] = P->geom[g]; A.flagged[g] = P->host_flagged[g]; }
    A.off[g + 1] = A.off[g] + (g < nh ? A.H[g].n : 0);
  }
  const int n = A.ntot = A.off[nh];
  if (hosts[nh]) { int rc = imm_resolve(ctx, *hosts[nh]); if (rc) return rc; }

  // the result blob (header | decisions | records) first, then what only the device sees
  size_t bytes = 0;
  auto take = [&](size_t b) { const size_t o = bytes; bytes += (b + 15) & ~(size_t)15; return o; };
  const size_t N = (size_t)n, nseg = (N + 255) / 256;
  const size_t o_hdr = take(sizeof(int) * ACT_H_INTS), o_dec = take(N), o_rec = take(sizeof(ImmActRec) * N);
  const size_t res_bytes = bytes;
  const size_t tab_floats = (size_t)nf * nf * 14;
  const size_t o_tab = take(sizeof(float) * tab_floats), o_img = take(sizeof(void*) * SDSO_IMM_MAX_HOSTS);
  const size_t tab_bytes = bytes - o_tab;
  const size_t o_flag = take(N), o_iu = take(4 * N), o_iv = take(4 * N), o_frac = take(4 * N), o_thr = take(4 * N), o_list = take(4 * N), o_pref = take(4 * N),
               o_back = take(4 * N), o_src = take(4 * N), o_seg = take(4 * (nseg + 1));
  int rc = ensure_scratch(ctx, bytes);
  if (rc) return rc;
  if (S.h_act_cap < res_bytes) {
    if (S.h_act) { SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream)); hipHostFree(S.h_act); S.h_act = nullptr; S.h_act_cap = 0; }
    const size_t want = (res_bytes * 3 / 2 + 4095) & ~(size_t)4095;
    SDSO_HIP(ctx, hipHostMalloc((void**)&S.h_act, want));
    S.h_act_cap = want;
  }
  S.act_valid = false;
  char* dp = (char*)ctx->scratch;
  int* d_hdr = (int*)(dp + o_hdr);
  uint8_t* d_dec = (uint8_t*)(dp + o_dec);
  int* h_hdr = (int*)S.h_act;
  for (int k = 0; k < ACT_H_INTS; k++) h_hdr[k] = 0;
  if (n) {
    char* stage = nullptr;
    rc = stage_reserve(ctx, S.stage, tab_bytes, &stage);
    if (rc) return rc;
    float* tf = (float*)stage;
    std::copy(P->pair_R, P->pair_R + (size_t)nf * nf * 9, tf);
    std::copy(P->pair_t, P->pair_t + (size_t)nf * nf * 3, tf + (size_t)nf * nf * 9);
    std::copy(P->pair_aff, P->pair_aff + (size_t)nf * nf * 2, tf + (size_t)nf * nf * 12);
    std::copy(imgs, imgs + SDSO_IMM_MAX_HOSTS, (const float4**)(stage + (o_img - o_tab)));
    SDSO_HIP(ctx, hipMemcpyAsync(dp + o_tab, stage, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = stage_commit(ctx, S.stage);
    if (rc) return rc;
    SDSO_HIP(ctx, hipMemsetAsync(d_hdr, 0, sizeof(int) * ACT_H_INTS, ctx->stream));
    uint8_t* d_flag = (uint8_t*)(dp + o_flag);
    int *d_iu = (int*)(dp + o_iu), *d_iv = (int*)(dp + o_iv), *d_list = (int*)(dp + o_list), *d_pref = (int*)(dp + o_pref), *d_back = (int*)(dp + o_back),
        *d_src = (int*)(dp + o_src), *d_seg = (int*)(dp + o_seg);
    float *d_frac = (float*)(dp + o_frac), *d_thr = (float*)(dp + o_thr);
    ImmActRec* d_rec = (ImmActRec*)(dp + o_rec);
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_act_classify", 2, k_imm_act_classify, g1, b1, A, P->currentMinActDist, P->minTraceQuality, w1, h1, d_dec, d_flag, d_iu, d_iv, d_frac, d_thr,
                 d_hdr);
    rc = dm_run_select(ctx, n, d_dec, d_iu, d_iv, d_frac, d_thr, 0, d_hdr + ACT_H_NSEL);
    if (rc) return rc;
    const ImmSelPred sp{d_dec};
    const ImmListEmit se{d_list};
    launch_timed(ctx, "k_imm_act_list", 2, k_imm_segcount<ImmSelPred>, dim3((unsigned)nseg), b1, sp, n, 256, d_seg);
    launch_timed(ctx, "k_imm_act_list", 2, k_imm_scan, dim3(1), b1, d_seg, (int)nseg, d_hdr + ACT_H_NLIST);
    launch_timed(ctx, "k_imm_act_list", 2, (k_imm_segwrite<ImmSelPred, ImmListEmit>), dim3((unsigned)nseg), b1, sp, se, n, 256, (const int*)d_seg);
    ActDev D = ActDev();
    D.nf = nf; D.w = P->w; D.h = P->h; D.n = 0; D.minObs = P->minObs;
    D.fx = P->K[0]; D.fy = P->K[1]; D.cx = P->K[2]; D.cy = P->K[3];
    D.pair_R = (const float*)(dp + o_tab); D.pair_t = D.pair_R + (size_t)nf * nf * 9; D.pair_aff = D.pair_R + (size_t)nf * nf * 12;
    D.img = (const float4* const*)(dp + o_img);
    launch_timed(ctx, "k_imm_activate", 1, k_imm_activate, dim3((n + 3) / 4), b1, A, D, (const int*)d_list, (const int*)(d_hdr + ACT_H_NLIST), d_rec, d_flag, d_hdr);
    launch_timed(ctx, "k_imm_act_prefix", 2, k_imm_act_prefix, dim3(nh), b1, A, (const uint8_t*)d_flag, d_pref, d_hdr);
    launch_timed(ctx, "k_imm_act_order", 2, k_imm_act_back, g1, b1, A, (const uint8_t*)d_flag, (const int*)d_pref, (const int*)d_hdr, d_back);
    launch_timed(ctx, "k_imm_act_order", 2, k_imm_act_src, g1, b1, A, (const uint8_t*)d_flag, (const int*)d_pref, (const int*)d_hdr, (const int*)d_back, d_src);
    const long threads = (long)n * (kImmFloats + 1);
    launch_timed(ctx, "k_imm_act_gather", 2, k_imm_act_gather, dim3((unsigned)((threads + 255) / 256)), b1, A, O, (const int*)d_hdr, (const int*)d_src);
    SDSO_HIP(ctx, hipGetLastError());
    // the one copy back: header, decisions and the first records; the list is longer than that only in windows the reference never builds
    const size_t first = std::min(N, (size_t)SDSO_IMM_ACT_FIRST_COPY);
    SDSO_HIP(ctx, hipMemcpyAsync(S.h_act, dp, o_rec + sizeof(ImmActRec) * first, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t nsel = (size_t)h_hdr[ACT_H_NLIST];
    if (nsel > first) {
      SDSO_HIP(ctx, hipMemcpyAsync(S.h_act + o_rec + sizeof(ImmActRec) * first, dp + o_rec + sizeof(ImmActRec) * first, sizeof(ImmActRec) * (nsel - first),
                                   hipMemcpyDeviceToHost, ctx->stream));
      SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int g = 0; g < nh; g++) {
      const int nflag = h_hdr[ACT_H_FLAGGED + g];
      if (!hosts[g] || nflag == 0) continue;
      hosts[g]->n -= nflag;
      std::swap(hosts[g]->f[0], hosts[g]->f[1]);
      std::swap(hosts[g]->st[0], hosts[g]->st[1]);
    }
  }
  S.act_valid = true; S.act_nf = nf; S.act_ntot = n; S.act_nsel = h_hdr[ACT_H_NLIST];
  if (counts) {
    for (int k = 0; k < SDSO_IMM_ACT_NCOUNTS; k++) counts[k] = 0;
    int removed = 0;
    for (int g = 0; g < nh; g++) removed += h_hdr[ACT_H_FLAGGED + g];
    counts[0] = n;
    counts[1] = n - h_hdr[ACT_H_DELETE] - h_hdr[ACT_H_NSEL]; counts[2] = h_hdr[ACT_H_DELETE]; counts[3] = h_hdr[ACT_H_NSEL];
    counts[4] = h_hdr[ACT_H_NLIST];
    for (int k = 0; k < 3; k++) counts[5 + k] = h_hdr[ACT_H_STATUS + k];
    counts[8] = removed;
    for (int f = 0; f < nf; f++) counts[9 + f] = hosts[f] ? hosts[f]->n : 0;
  }
  return SDSO_OK;
}

extern "C" int sdso_imm_activate_fetch(sdso_ctx* ctx, sdso_imm_activated_t* out, uint8_t* decision) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->imm || !ctx->imm->act_valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_imm_activate on this ctx yet");
  SDSO_REQUIRE(ctx, out, "null argument");
  const ImmState& S = *ctx->imm;
  const size_t N = (size_t)S.act_ntot;
  const size_t o_dec = sizeof(int) * ACT_H_INTS, o_rec = o_dec + ((N + 15) & ~(size_t)15);
  const int n = out->n = S.act_nsel, nf = out->nf = S.act_nf;
  if (decision && N) std::copy(S.h_act + o_dec, S.h_act + o_dec + N, (char*)decision);
  const ImmActRec* R = (const ImmActRec*)(S.h_act + o_rec);
  for (int p = 0; p < n; p++) {
    const ImmActRec& r = R[p];
    if (out->frame) out->frame[p] = r.frame;
    if (out->index) out->index[p] = r.index;
    if (out->status) out->status[p] = r.status;
    if (out->idepth) out->idepth[p] = r.idepth;
    if (out->res_state) for (int f = 0; f < nf; f++) out->res_state[(size_t)p * nf + f] = r.res_state[f];
    if (out->u) out->u[p] = r.u;
    if (out->v) out->v[p] = r.v;
    if (out->my_type) out->my_type[p] = r.my_type;
    if (out->idepth_min) out->idepth_min[p] = r.idepth_min;
    if (out->idepth_max) out->idepth_max[p] = r.idepth_max;
    if (out->energyTH) out->energyTH[p] = r.energyTH;
    if (out->color) for (int k = 0; k < 8; k++) out->color[(size_t)p * 8 + k] = r.color[k];
    if (out->weights) for (int k = 0; k < 8; k++) out->weights[(size_t)p * 8 + k] = r.weights[k];
    if (out->lastTraceStatus) out->lastTraceStatus[p] = r.lastTraceStatus;
  }
  return SDSO_OK;
}
