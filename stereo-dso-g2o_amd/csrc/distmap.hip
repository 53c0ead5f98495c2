// CoarseDistanceMap (src/FullSystem/CoarseTracker.cpp:1216-1372) and the candidate selection of FullSystem::activatePointsMT
// STEP 2 (src/FullSystem/FullSystem.cpp:837-902) on the device.
//
// The level-1 map lives in the ctx as BYTES: 0..39 = the step of growDistBFS that set the pixel, 255 = untouched (the reference's 1000).
//   k_distmap_seed   : project every active point (CoarseTracker.cpp:1242-1248), store 0 at the seeds, count them (numItems);
//                      k_distmap_seed_window: the same from the points of a resident BA window (sdso_distmap_make_from_window)
//   k_distmap_grow   : growDistBFS (:1260-1363) from scratch, one workgroup per 64x64 tile with a 39-pixel halo in LDS — a pixel's value
//                      depends only on seeds within 39 pixels and on paths inside that radius, so tiles never exchange anything
//   k_select_classify: the per-candidate gates of STEP 2 (FullSystem.cpp:850-887), independent per candidate
//   k_distmap_select : the order-dependent rest (:889-895): one workgroup holds the whole map in LDS, one wave walks the candidates in
//                      order, 64 at a time, and re-grows the map around every selected pixel as addIntoDistFinal does (:1366-1372)
#include "sdso_internal.h"
#include "distmap_dev.h"
#include <cmath>
#include <cstring>

using namespace sdso;

namespace sdso {

constexpr int DM_R = 39;                    // growDistBFS runs k = 1..39 (:1266)
constexpr int DM_T = 64;                    // tile edge of the from-scratch growth
constexpr int DM_S = DM_T + 2 * DM_R;       // 142: tile + halo; 142*142 = 20 164 B of LDS per workgroup
constexpr int DM_WIN = 2 * DM_R + 1;        // 79: an insert never leaves the 79x79 window around its seed
constexpr int DM_LDS_MAP = 144 * 1024;      // the selection kernel keeps maps up to this many pixels in LDS (616x184 = 113 344)
constexpr uint8_t DM_FAR = 255;             // untouched (1000 in the reference)
constexpr uint8_t DM_OUTSIDE = 254;         // halo pixel outside the image: never assigned, never propagates

struct DistMapState {
  int w1 = 0, h1 = 0;
  bool valid = false;          // a map has been made for (w1, h1)
  DevBuf<uint8_t> seed;        // w1*h1 bytes (padded to 16): 0 at the seeds, 255 elsewhere
  DevBuf<uint8_t> map;         // w1*h1 bytes (padded to 16)
  DevBuf<int> cnt;             // numItems of sdso_distmap_make_from_window (the host route counts in the ctx scratch)
  size_t cap = 0;              // bytes seed and map both hold
};

void release_distmap(sdso_ctx* ctx) {
  delete ctx->dm;
  ctx->dm = nullptr;
}

__global__ __launch_bounds__(256) void k_distmap_seed(int n, const sdso_distmap_geom_t* __restrict__ geom, const int* __restrict__ pg, const float* __restrict__ u,
                                                      const float* __restrict__ v, const float* __restrict__ idepth, int w1, int h1, uint8_t* __restrict__ seed,
                                                      int* __restrict__ n_seeds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (i < n) {
    int iu, iv;
    float p0;
    in = dm_project(geom[pg[i]], u[i], v[i], idepth[i], w1, h1, iu, iv, p0);
    if (in) seed[iu + w1 * iv] = 0;       // every writer stores 0
  }
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_seeds, __popcll(b));
}

// The same seeds from a device-resident BA window (sdso_distmap_make_from_window): point p of the window is projected with the geometry of
// its host frame, its u, v and its current idepth (p_geo.z: idepth_scaled, SCALE_IDEPTH = 1).  G holds the window's frames (at most 8) and
// travels as a kernel argument; skip[f] != 0: the points of frame f contribute nothing (`if (fh == frame) continue`, CoarseTracker.cpp:1232).
struct DmWinGeoms { sdso_distmap_geom_t G[8]; uint8_t skip[8]; };
__global__ __launch_bounds__(256) void k_distmap_seed_window(int n, int nf, const DmWinGeoms A, const float4* __restrict__ p_geo, const int* __restrict__ p_host,
                                                             int w1, int h1, uint8_t* __restrict__ seed, int* __restrict__ n_seeds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (i < n) {
    const int f = p_host[i];
    if (f >= 0 && f < nf && !A.skip[f]) {
      const float4 g = p_geo[i];
      int iu, iv;
      float p0;
      in = dm_project(A.G[f], g.x, g.y, g.z, w1, h1, iu, iv, p0);
      if (in) seed[iu + w1 * iv] = 0;     // every writer stores 0
    }
  }
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_seeds, __popcll(b));
}

// Level-synchronous form of growDistBFS: at step k an untouched pixel becomes k iff a neighbour — 8-neighbourhood for odd k, 4 for even k —
// holds exactly k-1 and is not on the map's outer border (:1279).  At step k only local coordinates [k, DM_S-k) can still reach the tile.
__global__ __launch_bounds__(256) void k_distmap_grow(const uint8_t* __restrict__ seed, uint8_t* __restrict__ map, int w1, int h1) {
  __shared__ uint8_t t[DM_S * DM_S];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = blockIdx.x * DM_T - DM_R, y0 = blockIdx.y * DM_T - DM_R;
  for (int ly = wv; ly < DM_S; ly += 4) {
    const int gy = y0 + ly;
    for (int lx = lane; lx < DM_S; lx += 64) {
      const int gx = x0 + lx;
      t[lx + DM_S * ly] = (gx >= 0 && gy >= 0 && gx < w1 && gy < h1) ? seed[gx + w1 * gy] : DM_OUTSIDE;
    }
  }
  __syncthreads();
  for (int k = 1; k <= DM_R; k++) {
    int changed = 0;
    const uint8_t prev = (uint8_t)(k - 1);
    for (int ly = k + wv; ly < DM_S - k; ly += 4) {
      const int gy = y0 + ly;
      for (int lx = k + lane; lx < DM_S - k; lx += 64) {
        const int p = lx + DM_S * ly;
        if (t[p] != DM_FAR) continue;
        const int gx = x0 + lx;
        // a neighbour (gx+dx, gy+dy) propagates iff it is strictly inside the map
        const bool cl = gx - 1 > 0 && gx - 1 < w1 - 1, cc = gx > 0 && gx < w1 - 1, cr = gx + 1 > 0 && gx + 1 < w1 - 1;
        const bool ru = gy - 1 > 0 && gy - 1 < h1 - 1, rc = gy > 0 && gy < h1 - 1, rd = gy + 1 > 0 && gy + 1 < h1 - 1;
        bool hit = (cl && rc && t[p - 1] == prev) || (cr && rc && t[p + 1] == prev) || (cc && ru && t[p - DM_S] == prev) || (cc && rd && t[p + DM_S] == prev);
        if (!hit && (k & 1))
          hit = (cl && ru && t[p - 1 - DM_S] == prev) || (cr && ru && t[p + 1 - DM_S] == prev) || (cl && rd && t[p - 1 + DM_S] == prev) ||
                (cr && rd && t[p + 1 + DM_S] == prev);
        if (hit) { t[p] = (uint8_t)k; changed = 1; }
      }
    }
    // nothing set in step k: the frontier is empty for good (__syncthreads_or is also the barrier of the step)
    if (!__syncthreads_or(changed)) break;
  }
  for (int ly = DM_R + wv; ly < DM_R + DM_T; ly += 4) {
    const int gy = y0 + ly, gx = x0 + DM_R + lane;
    if (gy < h1 && gx < w1) map[gx + w1 * gy] = t[DM_R + lane + DM_S * ly];
  }
}

// activatePointsMT STEP 2, the gates that do not depend on the map (FullSystem.cpp:850-887)
struct SelDev {
  int n, w1, h1;
  float minActDist, minTraceQuality;
  const sdso_distmap_geom_t* geom;
  const uint8_t* flagged;
  const int* pg;
  const float *u, *v, *imin, *imax, *quality, *interval, *my_type;
  const uint8_t* status;
  uint8_t* dec;
  int *iu, *iv;
  float *frac, *thr;
};
// one candidate of the uploaded arrays, for dm_classify
struct SelCand {
  const SelDev& S; int i, g;
  __device__ uint8_t status() const { return S.status[i]; }
  __device__ float imax() const { return S.imax[i]; }
  __device__ float imin() const { return S.imin[i]; }
  __device__ float interval() const { return S.interval[i]; }
  __device__ float quality() const { return S.quality[i]; }
  __device__ bool flagged() const { return S.flagged[g] != 0; }
  __device__ const sdso_distmap_geom_t& geom() const { return S.geom[g]; }
  __device__ float u() const { return S.u[i]; }
  __device__ float v() const { return S.v[i]; }
};
__global__ __launch_bounds__(256) void k_select_classify(SelDev S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  int iu = 0, iv = 0;
  float frac = 0.f;
  S.dec[i] = dm_classify(SelCand{S, i, S.pg[i]}, S.minTraceQuality, S.w1, S.h1, iu, iv, frac);
  S.iu[i] = iu;
  S.iv[i] = iv;
  S.frac[i] = frac;
  S.thr[i] = S.minActDist * S.my_type[i];                                            // :892
}

// the single wave of the selection kernel orders its own LDS / global accesses: a store of one lane must be seen by the loads that
// other lanes of the wave issue later
__device__ __forceinline__ void dm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// addIntoDistFinal(sx, sy) = growDistBFS(1) from one seed (:1366-1372) by ONE wave: only pixels newly set in step k-1 propagate in
// step k, a pixel is taken when its value is > k.  `list` receives every newly set pixel once, as an offset inside the 79x79 window
// around the seed (so 79*79 entries bound it); [beg, end) is the frontier of the previous step.  The eight directions are handled one
// after the other by the whole wave, so two frontier pixels never take the same neighbour: the second one already reads k.
template <class MapPtr>
__device__ __forceinline__ void dm_insert(MapPtr map, int w1, int h1, int sx, int sy, unsigned short* list, int lane) {
  constexpr int DX[8] = {1, -1, 0, 0, 1, -1, -1, 1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
  if (lane == 0) {
    map[sx + w1 * sy] = 0;
    list[0] = (unsigned short)(DM_R + DM_WIN * DM_R);
  }
  dm_wave_sync();
  int beg = 0, end = 1;
  for (int k = 1; k <= DM_R && beg < end; k++) {
    int cnt = end;
    for (int c = beg; c < end; c += 64) {
      const int e = c + lane;
      bool act = e < end;
      int x = 0, y = 0;
      if (act) {
        const int o = list[e];
        x = sx + o % DM_WIN - DM_R;
        y = sy + o / DM_WIN - DM_R;
        act = !(x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1);     // :1279
      }
#pragma unroll
      for (int d = 0; d < 8; d++) {
        if (d >= 4 && !(k & 1)) break;
        const int nx = x + DX[d], ny = y + DY[d];
        bool set = false;
        if (act) {
          const int idx = nx + w1 * ny;
          if (map[idx] > k) { map[idx] = (uint8_t)k; set = true; }
        }
        const unsigned long long b = __ballot(set);
        if (set) {
          const int pos = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0));
          list[pos] = (unsigned short)((nx - sx + DM_R) + DM_WIN * (ny - sy + DM_R));
        }
        cnt += __popcll(b);
        dm_wave_sync();
      }
    }
    beg = end;
    end = cnt;
  }
}

// The distance test and the re-growth, in candidate order.  The map only ever decreases, so a candidate that fails the test against
// the current map fails it against every later one: 64 candidates are tested at once, the failures are final (KEEP), the first lane
// that passes is the next one the reference's loop would select; after its insert the lanes behind it are tested again.
// mode_add: every entry is inserted unconditionally (sdso_distmap_add).
template <bool LDSMAP>
__global__ __launch_bounds__(256) void k_distmap_select(uint8_t* __restrict__ gmap, int w1, int h1, int n, uint8_t* __restrict__ dec, const int* __restrict__ iu,
                                                        const int* __restrict__ iv, const float* __restrict__ frac, const float* __restrict__ thr,
                                                        int mode_add, int* __restrict__ n_selected) {
  __shared__ __attribute__((aligned(16))) uint8_t smap[LDSMAP ? DM_LDS_MAP : 16];
  __shared__ unsigned short list[DM_WIN * DM_WIN];
  const int npix16 = (w1 * h1 + 15) >> 4;     // the device buffers are padded to 16 bytes
  if (LDSMAP) {
    for (int i = threadIdx.x; i < npix16; i += 256) ((uint4*)smap)[i] = ((const uint4*)gmap)[i];
    __syncthreads();
  }
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int nsel = 0;
    // candidate of this lane in the next chunk, requested one chunk ahead
    int i = lane;
    uint8_t d_n = (i < n) ? (mode_add ? (uint8_t)DM_PENDING : dec[i]) : (uint8_t)DM_KEEP;
    int x_n = (i < n) ? iu[i] : 0, y_n = (i < n) ? iv[i] : 0;
    float f_n = (i < n && !mode_add) ? frac[i] : 0.f, t_n = (i < n && !mode_add) ? thr[i] : 0.f;
    for (int base = 0; base < n; base += 64) {
      i = base + lane;
      const uint8_t d0 = d_n;
      const int x = x_n, y = y_n;
      const float f = f_n, t = t_n;
      const int j = i + 64;
      if (base + 64 < n) {
        d_n = (j < n) ? (mode_add ? (uint8_t)DM_PENDING : dec[j]) : (uint8_t)DM_KEEP;
        x_n = (j < n) ? iu[j] : 0; y_n = (j < n) ? iv[j] : 0;
        f_n = (j < n && !mode_add) ? frac[j] : 0.f; t_n = (j < n && !mode_add) ? thr[j] : 0.f;
      }
      bool alive = d0 == DM_PENDING;
      uint8_t out = DM_KEEP;
      const int idx = x + w1 * y;
      for (;;) {
        if (alive && !mode_add) {
          const uint8_t m = LDSMAP ? smap[idx] : gmap[idx];
          const float dist = (m == DM_FAR ? 1000.f : (float)m) + f;      // FullSystem.cpp:889
          if (!(dist >= t)) alive = false;                                // :892
        }
        const unsigned long long b = __ballot(alive);
        if (!b) break;
        const int first = __ffsll((long long)b) - 1;
        const int sx = __shfl(x, first, 64), sy = __shfl(y, first, 64);
        if (LDSMAP) dm_insert(smap, w1, h1, sx, sy, list, lane);
        else dm_insert(gmap, w1, h1, sx, sy, list, lane);
        if (lane == first) { alive = false; out = DM_SELECT; }
        nsel++;
      }
      if (!mode_add && d0 == DM_PENDING) dec[i] = out;
    }
    if (lane == 0 && n_selected) *n_selected = nsel;
  }
  if (LDSMAP) {
    __syncthreads();
    for (int i = threadIdx.x; i < npix16; i += 256) ((uint4*)gmap)[i] = ((const uint4*)smap)[i];
  }
}

static int dm_ensure(sdso_ctx* ctx, int w1, int h1) {
  if (!ctx->dm) ctx->dm = new DistMapState();
  DistMapState& D = *ctx->dm;
  const size_t need = (((size_t)w1 * h1 + 15) & ~(size_t)15) + 16;
  if (D.cap < need) {   // a group (devbuf.h)
    D.cap = 0; D.valid = false;
    SDSO_HIP(ctx, devbuf::reset_all(ctx->stream, D.seed, D.map));
    SDSO_HIP(ctx, D.seed.reserve(ctx->stream, need, need));
    SDSO_HIP(ctx, D.map.reserve(ctx->stream, need, need));
    D.cap = need;
  }
  SDSO_HIP(ctx, D.cnt.reserve(ctx->stream, 4, 4));
  if (D.w1 != w1 || D.h1 != h1) D.valid = false;
  D.w1 = w1; D.h1 = h1;
  return SDSO_OK;
}

// one staging block: host arrays are packed into pinned memory at 16-byte aligned offsets and go to the device scratch in one copy
struct Stage {
  size_t bytes = 0;
  size_t add(size_t b) { const size_t o = bytes; bytes += (b + 15) & ~(size_t)15; return o; }
};

int dm_run_select(sdso_ctx* ctx, int n, uint8_t* dec, const int* iu, const int* iv, const float* frac, const float* thr, int mode_add, int* n_selected) {
  DistMapState& D = *ctx->dm;
  if ((size_t)D.w1 * D.h1 <= (size_t)DM_LDS_MAP)
    launch_timed(ctx, "k_distmap_select", 1, k_distmap_select<true>, dim3(1), dim3(256), D.map, D.w1, D.h1, n, dec, iu, iv, frac, thr, mode_add, n_selected);
  else
    launch_timed(ctx, "k_distmap_select", 1, k_distmap_select<false>, dim3(1), dim3(256), D.map, D.w1, D.h1, n, dec, iu, iv, frac, thr, mode_add, n_selected);
  SDSO_HIP(ctx, hipGetLastError());
  return SDSO_OK;
}

bool distmap_dims(sdso_ctx* ctx, int* w1, int* h1) {
  if (!ctx->dm || !ctx->dm->valid) return false;
  *w1 = ctx->dm->w1; *h1 = ctx->dm->h1;
  return true;
}

}  // namespace sdso

// ------------------------------------------------------------------ API
extern "C" int sdso_distmap_make(sdso_ctx* ctx, int w, int h, int ngeom, const sdso_distmap_geom_t* geom, int n, const int* point_geom, const float* u,
                                 const float* v, const float* idepth_scaled, int* n_seeds) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, w >= 16 && h >= 16 && w <= 32768 && h <= 32768, "image size out of range");
  SDSO_REQUIRE(ctx, n >= 0 && ngeom >= 0 && (n == 0 || (ngeom > 0 && geom && point_geom && u && v && idepth_scaled)), "null argument");
  for (int i = 0; i < n; i++) SDSO_REQUIRE(ctx, point_geom[i] >= 0 && point_geom[i] < ngeom, "point_geom out of range");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const int w1 = w >> 1, h1 = h >> 1;
  int rc = dm_ensure(ctx, w1, h1);
  if (rc) return rc;
  DistMapState& D = *ctx->dm;
  D.valid = false;
  Stage S;
  const size_t o_cnt = S.add(sizeof(int)), o_geom = S.add(sizeof(sdso_distmap_geom_t) * (size_t)ngeom), o_pg = S.add(sizeof(int) * (size_t)n),
               o_u = S.add(sizeof(float) * (size_t)n), o_v = S.add(sizeof(float) * (size_t)n), o_id = S.add(sizeof(float) * (size_t)n);
  if ((rc = ensure_pinned(ctx, S.bytes))) return rc;
  if ((rc = ensure_scratch(ctx, S.bytes))) return rc;
  char* hp = (char*)ctx->pinned;
  char* dp = (char*)ctx->scratch;
  *(int*)(hp + o_cnt) = 0;
  if (n) {
    std::memcpy(hp + o_geom, geom, sizeof(sdso_distmap_geom_t) * (size_t)ngeom);
    std::memcpy(hp + o_pg, point_geom, sizeof(int) * (size_t)n);
    std::memcpy(hp + o_u, u, sizeof(float) * (size_t)n);
    std::memcpy(hp + o_v, v, sizeof(float) * (size_t)n);
    std::memcpy(hp + o_id, idepth_scaled, sizeof(float) * (size_t)n);
  }
  SDSO_HIP(ctx, hipMemcpyAsync(dp, hp, S.bytes, hipMemcpyHostToDevice, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(D.seed, DM_FAR, D.cap, ctx->stream));
  if (n)
    launch_timed(ctx, "k_distmap_seed", 2, k_distmap_seed, dim3((n + 255) / 256), dim3(256), n, (const sdso_distmap_geom_t*)(dp + o_geom), (const int*)(dp + o_pg),
                 (const float*)(dp + o_u), (const float*)(dp + o_v), (const float*)(dp + o_id), w1, h1, D.seed, (int*)(dp + o_cnt));
  launch_timed(ctx, "k_distmap_grow", 1, k_distmap_grow, dim3((w1 + DM_T - 1) / DM_T, (h1 + DM_T - 1) / DM_T), dim3(256), (const uint8_t*)D.seed, D.map, w1, h1);
  SDSO_HIP(ctx, hipGetLastError());
  SDSO_HIP(ctx, hipMemcpyAsync(hp + o_cnt, dp + o_cnt, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_seeds) *n_seeds = *(int*)(hp + o_cnt);
  D.valid = true;
  return SDSO_OK;
}

// makeDistanceMap on the points of a resident window.  The reference walks frameHessians and each frame's pointHessians (:1231-1249); the
// window keeps its points in exactly that order (makeIDX), but the order does not matter anyway: every seed stores the same 0 and numItems
// only counts, so any order of the same points gives the same seed image, and k_distmap_grow starts from that image alone.
extern "C" int sdso_distmap_make_from_window(sdso_ctx* ctx, int win, int w, int h, const sdso_distmap_geom_t* geom, const uint8_t* skip, int* n_seeds) {
  if (!ctx) return SDSO_ERR_STATE;
  BaPointsView V;
  SDSO_TRY(ba_window_points(ctx, win, &V));
  SDSO_REQUIRE(ctx, w >= 16 && h >= 16 && w <= 32768 && h <= 32768, "image size out of range");
  SDSO_REQUIRE(ctx, w == V.w && h == V.h, "w / h differ from the window's");
  SDSO_REQUIRE(ctx, geom, "null argument");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const int w1 = w >> 1, h1 = h >> 1;
  SDSO_TRY(dm_ensure(ctx, w1, h1));
  DistMapState& D = *ctx->dm;
  D.valid = false;
  DmWinGeoms A;
  std::memset(&A, 0, sizeof(A));
  for (int f = 0; f < V.nf; f++) { A.G[f] = geom[f]; A.skip[f] = skip && skip[f] ? 1 : 0; }
  int* d_cnt = D.cnt;
  SDSO_HIP(ctx, hipMemsetAsync(D.seed, DM_FAR, D.cap, ctx->stream));
  SDSO_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int), ctx->stream));
  if (V.np)
    launch_timed(ctx, "k_distmap_seed_window", 2, k_distmap_seed_window, dim3((V.np + 255) / 256), dim3(256), V.np, V.nf, A, V.p_geo, V.p_host, w1, h1, D.seed, d_cnt);
  launch_timed(ctx, "k_distmap_grow", 1, k_distmap_grow, dim3((w1 + DM_T - 1) / DM_T, (h1 + DM_T - 1) / DM_T), dim3(256), (const uint8_t*)D.seed, D.map, w1, h1);
  SDSO_HIP(ctx, hipGetLastError());
  if (n_seeds) {
    SDSO_TRY(ensure_pinned(ctx, sizeof(int)));
    SDSO_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_cnt, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_seeds = *(int*)ctx->pinned;
  }
  D.valid = true;
  return SDSO_OK;
}

extern "C" int sdso_distmap_add(sdso_ctx* ctx, int n, const int* iu, const int* iv) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->dm || !ctx->dm->valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no distance map yet (sdso_distmap_make)");
  SDSO_REQUIRE(ctx, n >= 0 && (n == 0 || (iu && iv)), "null argument");
  DistMapState& D = *ctx->dm;
  for (int i = 0; i < n; i++) SDSO_REQUIRE(ctx, iu[i] >= 0 && iv[i] >= 0 && iu[i] < D.w1 && iv[i] < D.h1, "pixel outside the level-1 map");
  if (n == 0) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  Stage S;
  const size_t o_u = S.add(sizeof(int) * (size_t)n), o_v = S.add(sizeof(int) * (size_t)n);
  int rc;
  if ((rc = ensure_pinned(ctx, S.bytes))) return rc;
  if ((rc = ensure_scratch(ctx, S.bytes))) return rc;
  char* hp = (char*)ctx->pinned;
  char* dp = (char*)ctx->scratch;
  std::memcpy(hp + o_u, iu, sizeof(int) * (size_t)n);
  std::memcpy(hp + o_v, iv, sizeof(int) * (size_t)n);
  SDSO_HIP(ctx, hipMemcpyAsync(dp, hp, S.bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = dm_run_select(ctx, n, nullptr, (const int*)(dp + o_u), (const int*)(dp + o_v), nullptr, nullptr, 1, nullptr))) return rc;
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

extern "C" int sdso_distmap_get(sdso_ctx* ctx, float* map) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->dm || !ctx->dm->valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no distance map yet (sdso_distmap_make)");
  SDSO_REQUIRE(ctx, map, "null argument");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  DistMapState& D = *ctx->dm;
  const size_t npix = (size_t)D.w1 * D.h1;
  int rc = ensure_pinned(ctx, npix);
  if (rc) return rc;
  SDSO_HIP(ctx, hipMemcpyAsync(ctx->pinned, D.map, npix, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint8_t* b = (const uint8_t*)ctx->pinned;
  for (size_t i = 0; i < npix; i++) map[i] = b[i] == DM_FAR ? 1000.f : (float)b[i];
  return SDSO_OK;
}

extern "C" int sdso_activate_select(sdso_ctx* ctx, const sdso_activate_select_t* A, uint8_t* decision, int* iu, int* iv, int* n_selected) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->dm || !ctx->dm->valid) return sdso::fail(ctx, SDSO_ERR_STATE, "no distance map yet (sdso_distmap_make)");
  SDSO_REQUIRE(ctx, A && A->n >= 0 && A->ngeom >= 0, "bad arguments");
  DistMapState& D = *ctx->dm;
  SDSO_REQUIRE(ctx, (A->w >> 1) == D.w1 && (A->h >> 1) == D.h1, "image size differs from the distance map's");
  const int n = A->n, ng = A->ngeom;
  if (n_selected) *n_selected = 0;
  if (n == 0) return SDSO_OK;
  SDSO_REQUIRE(ctx, decision && ng > 0 && A->geom && A->host_flagged && A->point_geom && A->u && A->v && A->idepth_min && A->idepth_max && A->quality &&
                        A->lastTracePixelInterval && A->lastTraceStatus && A->my_type, "null argument");
  for (int i = 0; i < n; i++) SDSO_REQUIRE(ctx, A->point_geom[i] >= 0 && A->point_geom[i] < ng, "point_geom out of range");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  // inputs first (one copy down), then the outputs dec | iu | iv | nsel (one copy up), then device-only frac | thr
  Stage S;
  const size_t o_geom = S.add(sizeof(sdso_distmap_geom_t) * (size_t)ng), o_flag = S.add((size_t)ng), o_pg = S.add(sizeof(int) * (size_t)n);
  size_t o_f[7];
  for (int k = 0; k < 7; k++) o_f[k] = S.add(sizeof(float) * (size_t)n);
  const size_t o_st = S.add((size_t)n);
  const size_t in_bytes = S.bytes;
  const size_t o_dec = S.add((size_t)n), o_iu = S.add(sizeof(int) * (size_t)n), o_iv = S.add(sizeof(int) * (size_t)n), o_ns = S.add(sizeof(int));
  const size_t out_end = S.bytes;
  const size_t o_frac = S.add(sizeof(float) * (size_t)n), o_thr = S.add(sizeof(float) * (size_t)n);
  int rc;
  if ((rc = ensure_pinned(ctx, out_end))) return rc;
  if ((rc = ensure_scratch(ctx, S.bytes))) return rc;
  char* hp = (char*)ctx->pinned;
  char* dp = (char*)ctx->scratch;
  std::memcpy(hp + o_geom, A->geom, sizeof(sdso_distmap_geom_t) * (size_t)ng);
  std::memcpy(hp + o_flag, A->host_flagged, (size_t)ng);
  std::memcpy(hp + o_pg, A->point_geom, sizeof(int) * (size_t)n);
  const float* fsrc[7] = {A->u, A->v, A->idepth_min, A->idepth_max, A->quality, A->lastTracePixelInterval, A->my_type};
  for (int k = 0; k < 7; k++) std::memcpy(hp + o_f[k], fsrc[k], sizeof(float) * (size_t)n);
  std::memcpy(hp + o_st, A->lastTraceStatus, (size_t)n);
  SDSO_HIP(ctx, hipMemcpyAsync(dp, hp, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  SelDev P;
  P.n = n; P.w1 = D.w1; P.h1 = D.h1; P.minActDist = A->currentMinActDist; P.minTraceQuality = A->minTraceQuality;
  P.geom = (const sdso_distmap_geom_t*)(dp + o_geom); P.flagged = (const uint8_t*)(dp + o_flag); P.pg = (const int*)(dp + o_pg);
  P.u = (const float*)(dp + o_f[0]); P.v = (const float*)(dp + o_f[1]); P.imin = (const float*)(dp + o_f[2]); P.imax = (const float*)(dp + o_f[3]);
  P.quality = (const float*)(dp + o_f[4]); P.interval = (const float*)(dp + o_f[5]); P.my_type = (const float*)(dp + o_f[6]);
  P.status = (const uint8_t*)(dp + o_st);
  P.dec = (uint8_t*)(dp + o_dec); P.iu = (int*)(dp + o_iu); P.iv = (int*)(dp + o_iv); P.frac = (float*)(dp + o_frac); P.thr = (float*)(dp + o_thr);
  launch_timed(ctx, "k_select_classify", 2, k_select_classify, dim3((n + 255) / 256), dim3(256), P);
  if ((rc = dm_run_select(ctx, n, P.dec, P.iu, P.iv, P.frac, P.thr, 0, (int*)(dp + o_ns)))) return rc;
  SDSO_HIP(ctx, hipMemcpyAsync(hp + o_dec, dp + o_dec, out_end - o_dec, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(decision, hp + o_dec, (size_t)n);
  if (iu) std::memcpy(iu, hp + o_iu, sizeof(int) * (size_t)n);
  if (iv) std::memcpy(iv, hp + o_iv, sizeof(int) * (size_t)n);
  if (n_selected) *n_selected = *(int*)(hp + o_ns);
  return SDSO_OK;
}
