// The device-resident map (gfx950): the records of every keyframe's pointHessians, pointHessiansMarginalized and pointHessiansOut, filled from
// the resident BA window while its post-state is valid, and KeyFrameDisplay::setFromKF / refreshPC on them.  Every rule that decides a byte
// is in map_cloud.h.
//
// Reference:
//   src/FullSystem/FullSystem.cpp:1467, src/FullSystem/FullSystemMarginalize.cpp:184   publishKeyframes, the two places the map is published
//   src/IOWrapper/Pangolin/KeyFrameDisplay.cpp:85-165                                  setFromKF: k_map_gather writes its records once, when
//                                                                                      the point's values are final for the keyframe
//   src/IOWrapper/Pangolin/KeyFrameDisplay.cpp:174-295                                 refreshPC: k_map_mark + k_map_emit
//
// The work is a few thousand to ~16 k records of 64 B in and at most 120 B out per kept point: launch- and latency-bound, nothing here is
// tuned for bandwidth.  What has to be right is the ORDER of the packed output:
//   k_map_gather  one lane per record: the ordered gather window -> lists (the host supplies the orders, sdso_abi.h says why)
//   k_map_mark    one lane per record of the query; every list starts a new wave, so a wave lies in one list of one frame.  The keep test
//                 per lane, one ballot per wave: the wave's mask is all the second kernel needs.  Kept points per list: integer atomics.
//   k_map_emit    the exclusive scan of the waves' popcounts in front of the workgroup (an integer block sum, the same on every run), then
//                 each kept lane writes its 8 vertices and colours at its offset.  No float atomics, no arrival order anywhere.
#include "ba_kernels.h"
#include "imm_layout.h"
#include "map_cloud.h"
#include <algorithm>
#include <cstring>

namespace sdso {

constexpr int MAP_BLOCK = 256;
constexpr int MAP_MAX_FRAMES = 8;                    // frames of one window / of one sdso_map_cloud
constexpr int MAP_MAX_SEGS = MAP_MAX_FRAMES * 4;     // cloud: immature, active, marginalised, out per frame
constexpr int MAP_NLIST = 3;

struct MapList {
  DevBuf<float> d;
  int n = 0;
  int cap() const { return (int)(d.cap() / MAP_REC_FLOATS); }   // records
};
struct MapKeyframe { MapList list[MAP_NLIST]; };     // [status - 1]
// one destination of k_map_gather: items [begin, next begin) go to dst + (item - begin) records
struct MapGatherSeg { float* dst; int begin, pad; };
struct MapGatherArgs { MapGatherSeg seg[MAP_MAX_FRAMES * MAP_NLIST + 1]; int nseg, n; };
// one list of a cloud query.  Waves [wbeg, next wbeg) hold its n records; cap > 0: an immature group's blob with that stride
struct MapCloudSeg { const float* src; int n, cap, status, frame, wbeg, pad; };
struct MapQuery {
  MapCloudSeg seg[MAP_MAX_SEGS + 1];
  float T[MAP_MAX_FRAMES][12];
  MapCalib K;
  float scaledTH, absTH, minBS;
  int mode, nseg, nwaves, world;
};
struct MapState {
  std::map<int, MapKeyframe> kf;
  StageBuf stage;
  DevBuf<int> d_idx;                                  // the staged point indices of sdso_map_update
  // sdso_map_cloud: [MapQuery | seg_kept MAP_MAX_SEGS ints | masks nwaves x 8 B] and the two output arrays
  DevBuf<char> d_work;
  DevBuf<float> d_xyz;
  DevBuf<uint8_t> d_rgb;
  int cloud_n = -1;                                   // vertices of the latest call; -1: none yet
};
static MapState& map_state(sdso_ctx* ctx) { if (!ctx->map) ctx->map = new MapState(); return *ctx->map; }
static MapKeyframe* map_find(sdso_ctx* ctx, int frameID) {
  if (!ctx->map) return nullptr;
  auto it = ctx->map->kf.find(frameID);
  return it == ctx->map->kf.end() ? nullptr : &it->second;
}
void release_map(sdso_ctx* ctx) {
  if (!ctx->map) return;
  stage_free(ctx->map->stage);
  delete ctx->map;
  ctx->map = nullptr;
}
// room for `want` records, the first `keep` of them carried over.  A list that grows is allocated anew (doubling) and copied device to
// device; the old block is freed once the stream has drained, since launches that read it may still be in flight.  The new block is `d`'s
// until then: a failure on the way frees it.
static int map_reserve(sdso_ctx* ctx, MapList& L, int want, int keep) {
  if (want <= L.cap()) return SDSO_OK;
  const size_t floats = MAP_REC_FLOATS * (size_t)std::max(std::max(want, 2 * L.cap()), 64);
  DevBuf<float> d;
  SDSO_HIP(ctx, d.reserve(ctx->stream, floats, floats));
  if (keep) SDSO_HIP(ctx, hipMemcpyAsync(d, L.d, sizeof(float) * MAP_REC_FLOATS * (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
  if (L.d) SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  L.d = std::move(d);
  return SDSO_OK;
}

// ------------------------------------------------------------------ kernels
// Item i of the call is window point idx[i]; its record goes to the list that owns item i, at its place in the given order.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_gather(const BaDev* __restrict__ win, const int* __restrict__ idx, MapGatherArgs A) {
  const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
  if (i >= A.n) return;
  const BaDev& B = *win;
  int s = 0;
  while (s + 1 < A.nseg && i >= A.seg[s + 1].begin) s++;
  const int p = gld(idx + i);
  const f32x4 geo = gld((const f32x4*)B.p_geo + p);            // u, v, idepth, idepth_zero
  const f32x4 tr = gld((const f32x4*)B.p_track + p);           // x maxRelBaseline, z idepth_hessian
  const f32x4 c0 = gld((const f32x4*)B.p_color + (size_t)p * 2), c1 = gld((const f32x4*)B.p_color + (size_t)p * 2 + 1);
  f32x4* out = (f32x4*)(A.seg[s].dst + (size_t)(i - A.seg[s].begin) * MAP_REC_FLOATS);
  gst(out + 0, f32x4{geo.x, geo.y, geo.z, tr.z});
  gst(out + 1, f32x4{tr.x, c0.x, c0.y, c0.z});
  gst(out + 2, f32x4{c0.w, c1.x, c1.y, c1.z});
  gst(out + 3, f32x4{c1.w, 0.f, 0.f, 0.f});
}

// the wave's list, found once per wave (nseg <= 32 scalar compares); w < Q.nwaves
__device__ __forceinline__ int map_seg_of_wave(const MapQuery& Q, int w) {
  int s = 0;
  while (s + 1 < uld(&Q.nseg) && w >= uld(&Q.seg[s + 1].wbeg)) s++;
  return __builtin_amdgcn_readfirstlane(s);
}
// what refreshPC reads of record i of a list: the record itself (four 16-byte loads), or the members of an immature point (:104-117)
struct MapPoint { float u, v, idepth, idh, bs, color[8]; };
__device__ __forceinline__ MapPoint map_load(const float* __restrict__ src, int cap, int i) {
  MapPoint P;
  if (cap > 0) {
    const size_t N = (size_t)cap;
    P.u = gld(src + IMM_U * N + i); P.v = gld(src + IMM_V * N + i);
    P.idepth = map_immature_idepth(gld(src + IMM_IMIN * N + i), gld(src + IMM_IMAX * N + i));
    P.idh = MAP_IMMATURE_IDH; P.bs = MAP_IMMATURE_BS;
#pragma unroll
    for (int k = 0; k < 8; k++) P.color[k] = gld(src + IMM_COLOR * N + (size_t)i * 8 + k);   // (the member starts 24 * cap bytes in: no 16-byte loads)
    return P;
  }
  const f32x4* r = (const f32x4*)(src + (size_t)i * MAP_REC_FLOATS);
  const f32x4 a = gld(r), b = gld(r + 1), c = gld(r + 2), d = gld(r + 3);
  P.u = a.x; P.v = a.y; P.idepth = a.z; P.idh = a.w; P.bs = b.x;
  P.color[0] = b.y; P.color[1] = b.z; P.color[2] = b.w; P.color[3] = c.x; P.color[4] = c.y; P.color[5] = c.z; P.color[6] = c.w; P.color[7] = d.x;
  return P;
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_mark(const MapQuery* __restrict__ query, int* __restrict__ seg_kept, unsigned long long* __restrict__ mask) {
  const MapQuery& Q = *query;
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (MAP_BLOCK / 64) + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (w >= uld(&Q.nwaves)) return;                            // (wave-uniform)
  const int s = map_seg_of_wave(Q, w);
  const int i = (w - uld(&Q.seg[s].wbeg)) * 64 + lane, n = uld(&Q.seg[s].n), cap = uld(&Q.seg[s].cap);
  bool keep = false;
  if (i < n) {
    const float* src = uld(&Q.seg[s].src);
    float idepth, idh, bs;
    if (cap > 0) {
      const size_t N = (size_t)cap;
      idepth = map_immature_idepth(gld(src + IMM_IMIN * N + i), gld(src + IMM_IMAX * N + i));
      idh = MAP_IMMATURE_IDH; bs = MAP_IMMATURE_BS;
    } else {
      const f32x4* r = (const f32x4*)(src + (size_t)i * MAP_REC_FLOATS);
      const f32x4 a = gld(r);
      idepth = a.z; idh = a.w; bs = gld(src + (size_t)i * MAP_REC_FLOATS + MAP_BS);
    }
    keep = map_keep(uld(&Q.seg[s].status), idepth, idh, bs, uld(&Q.mode), uld(&Q.scaledTH), uld(&Q.absTH), uld(&Q.minBS));
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) {
    gst(mask + w, m);
    if (m) atomicAdd(seg_kept + s, __popcll(m));
  }
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_emit(const MapQuery* __restrict__ query, const unsigned long long* __restrict__ mask, float* __restrict__ xyz,
                                                        uint8_t* __restrict__ rgb) {
  const MapQuery& Q = *query;
  __shared__ int s_part[MAP_BLOCK / 64];
  __shared__ int s_own[MAP_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
  const int w0 = blockIdx.x * (MAP_BLOCK / 64), w = __builtin_amdgcn_readfirstlane(w0 + wib), nwaves = uld(&Q.nwaves);
  // ---- kept points in front of this workgroup: an integer sum, whatever its order
  int before = 0;
  for (int j = tid; j < w0; j += MAP_BLOCK) before += __popcll(gld(mask + j));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  const unsigned long long m = w < nwaves ? gld(mask + w) : 0ull;   // (wave-uniform)
  if (lane == 0) { s_part[wib] = before; s_own[wib] = __popcll(m); }
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int k = 0; k < MAP_BLOCK / 64; k++) base += s_part[k] + (k < wib ? s_own[k] : 0);
  if (!((m >> lane) & 1ull)) return;
  const int pos = base + __popcll(m & ((1ull << lane) - 1ull));     // the point's place among the kept points of the call
  const int s = map_seg_of_wave(Q, w);
  const int i = (w - uld(&Q.seg[s].wbeg)) * 64 + lane;
  const MapPoint P = map_load(uld(&Q.seg[s].src), uld(&Q.seg[s].cap), i);
  const int status = uld(&Q.seg[s].status), mode = uld(&Q.mode), frame = uld(&Q.seg[s].frame), world = uld(&Q.world);
  const MapCalib K{uld(&Q.K.fxi), uld(&Q.K.fyi), uld(&Q.K.cxi), uld(&Q.K.cyi)};
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = world ? uld(&Q.T[frame][k]) : 0.f;
  const float depth = 1.0f / P.idepth;                               // :222
  float V[MAP_PATTERN * 3];
  uint8_t Cb[MAP_PATTERN * 3];
#pragma unroll
  for (int k = 0; k < MAP_PATTERN; k++) {
    int dx, dy;
    map_pattern(k, &dx, &dy);
    float cam[3];
    map_vertex(P.u, P.v, depth, dx, dy, K.fxi, K.fyi, K.cxi, K.cyi, cam);
    if (world) map_to_world(T, cam, &V[3 * k]);
    else { V[3 * k] = cam[0]; V[3 * k + 1] = cam[1]; V[3 * k + 2] = cam[2]; }
    map_colour(status, mode, P.color[k], &Cb[3 * k]);
  }
  // 96 B of vertices and 24 B of colours per point, both at a multiple of their size
  f32x4* ov = (f32x4*)(xyz + (size_t)pos * MAP_PATTERN * 3);
#pragma unroll
  for (int k = 0; k < 6; k++) gst(ov + k, f32x4{V[4 * k], V[4 * k + 1], V[4 * k + 2], V[4 * k + 3]});
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  u32x2* oc = (u32x2*)(rgb + (size_t)pos * MAP_PATTERN * 3);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) { lo |= (unsigned)Cb[8 * k + b] << (8 * b); hi |= (unsigned)Cb[8 * k + 4 + b] << (8 * b); }
    gst(oc + k, u32x2{lo, hi});
  }
}

static bool map_list_ok(int list) { return list >= MAP_ST_ACTIVE && list <= MAP_ST_OUT; }

}  // namespace sdso

using namespace sdso;

// ------------------------------------------------------------------ the store
extern "C" int sdso_map_update(sdso_ctx* ctx, int win, const sdso_map_update_t* U) {
  if (!ctx) return SDSO_ERR_STATE;
  // ---- refusals: all before any device work
  BaRefView V;
  SDSO_TRY(ba_ref_view(ctx, win, &V));
  SDSO_REQUIRE(ctx, U, "null sdso_map_update_t");
  const int nf = V.nf, np = V.np;
  SDSO_REQUIRE(ctx, U->n_gone >= 0 && (U->n_gone == 0 || (U->gone && U->gone_list)), "n_gone without gone / gone_list");
  SDSO_REQUIRE(ctx, U->active == nullptr || U->n_active >= 0, "negative n_active");
  SDSO_REQUIRE(ctx, nf <= MAP_MAX_FRAMES, "the window holds more than 8 frames");
  std::vector<uint8_t> seen((size_t)np, 0);
  for (int k = 0; k < U->n_gone; k++) {
    SDSO_REQUIRE(ctx, U->gone_list[k] == MAP_ST_MARGINALIZED || U->gone_list[k] == MAP_ST_OUT, "gone_list entry other than 2 (marginalised) or 3 (out)");
    SDSO_REQUIRE(ctx, U->gone[k] >= 0 && U->gone[k] < np, "gone: point index out of range");
    SDSO_REQUIRE(ctx, !seen[U->gone[k]], "gone: point named twice");
    seen[U->gone[k]] = 1;
  }
  if (U->active) {
    for (int k = 0; k < U->n_active; k++) {
      SDSO_REQUIRE(ctx, U->active[k] >= 0 && U->active[k] < np, "active: point index out of range");
      SDSO_REQUIRE(ctx, !seen[U->active[k]], "active: point named twice (in active, or in active and gone)");
      seen[U->active[k]] = 1;
    }
    SDSO_REQUIRE(ctx, U->n_active + U->n_gone == np, "n_active + n_gone differs from the window's points");
  }
  int frameID[8], pt_beg[9];
  SDSO_TRY(ba_window_hosts(ctx, win, frameID, pt_beg));
  for (int a = 0; a < nf; a++)
    for (int b = a + 1; b < nf; b++) SDSO_REQUIRE(ctx, frameID[a] != frameID[b], "two frames of the window share a frameID");
  // ---- the items, list by list: per frame its active points, then what joins its marginalised and its out list, each in the given order
  std::vector<int> host((size_t)np);
  for (int h = 0; h < nf; h++) for (int p = pt_beg[h]; p < pt_beg[h + 1]; p++) host[p] = h;
  std::vector<int> item[MAP_MAX_FRAMES][MAP_NLIST];
  if (U->active) { for (int k = 0; k < U->n_active; k++) item[host[U->active[k]]][0].push_back(U->active[k]); }
  else { for (int p = 0; p < np; p++) if (!seen[p]) item[host[p]][0].push_back(p); }
  for (int k = 0; k < U->n_gone; k++) item[host[U->gone[k]]][U->gone_list[k] - 1].push_back(U->gone[k]);
  // ---- device work
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  MapState& S = map_state(ctx);
  MapGatherArgs A;
  std::memset(&A, 0, sizeof(A));
  std::vector<int> idx;
  // A failure of the device phase leaves the map as it was too: room is made first (a list that grows keeps its records and its size),
  // the new sizes are committed once the gather is enqueued, and a keyframe this call created goes again if it does not get that far.
  int new_n[MAP_MAX_FRAMES][MAP_NLIST];
  std::vector<int> created;
  auto enqueue = [&]() -> int {
    for (int h = 0; h < nf; h++) {
      if (S.kf.find(frameID[h]) == S.kf.end()) created.push_back(frameID[h]);
      MapKeyframe& K = S.kf[frameID[h]];                     // created by the first update that names it
      for (int l = 0; l < MAP_NLIST; l++) {
        MapList& L = K.list[l];
        const int add = (int)item[h][l].size(), keep = l == 0 ? 0 : L.n;   // the active list is replaced, the other two are appended to
        SDSO_TRY(map_reserve(ctx, L, keep + add, L.n));
        new_n[h][l] = keep + add;
        if (!add) continue;
        A.seg[A.nseg++] = MapGatherSeg{L.d + (size_t)keep * MAP_REC_FLOATS, (int)idx.size(), 0};
        idx.insert(idx.end(), item[h][l].begin(), item[h][l].end());
      }
    }
    A.n = (int)idx.size();
    A.seg[A.nseg] = MapGatherSeg{nullptr, A.n, 0};
    if (!A.n) return SDSO_OK;
    SDSO_HIP(ctx, S.d_idx.reserve(ctx->stream, (size_t)A.n, (size_t)A.n + (size_t)A.n / 2 + 64));
    char* stage = nullptr;
    SDSO_TRY(stage_reserve(ctx, S.stage, sizeof(int) * (size_t)A.n, &stage));
    std::memcpy(stage, idx.data(), sizeof(int) * (size_t)A.n);
    SDSO_HIP(ctx, hipMemcpyAsync(S.d_idx, stage, sizeof(int) * (size_t)A.n, hipMemcpyHostToDevice, ctx->stream));
    SDSO_TRY(stage_commit(ctx, S.stage));
    launch_timed(ctx, "k_map_gather", 2, k_map_gather, dim3((A.n + MAP_BLOCK - 1) / MAP_BLOCK), dim3(MAP_BLOCK), V.dev, (const int*)S.d_idx, A);
    SDSO_HIP(ctx, hipGetLastError());
    return SDSO_OK;
  };
  const int rc = enqueue();
  if (rc) {
    for (int id : created) S.kf.erase(id);
    return rc;
  }
  for (int h = 0; h < nf; h++) for (int l = 0; l < MAP_NLIST; l++) S.kf[frameID[h]].list[l].n = new_n[h][l];
  return SDSO_OK;
}

extern "C" int sdso_map_counts(sdso_ctx* ctx, int frameID, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, counts, "null counts");
  const MapKeyframe* K = map_find(ctx, frameID);
  SDSO_REQUIRE(ctx, K, "unknown frameID");
  for (int l = 0; l < MAP_NLIST; l++) counts[l] = K->list[l].n;
  return SDSO_OK;
}

extern "C" int sdso_map_get(sdso_ctx* ctx, int frameID, int list, float* records) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, map_list_ok(list), "list other than 1 (active), 2 (marginalised) or 3 (out)");
  const MapKeyframe* K = map_find(ctx, frameID);
  SDSO_REQUIRE(ctx, K, "unknown frameID");
  const MapList& L = K->list[list - 1];
  if (!L.n) return SDSO_OK;
  SDSO_REQUIRE(ctx, records, "null records");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipMemcpyAsync(records, L.d, sizeof(float) * MAP_REC_FLOATS * (size_t)L.n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

extern "C" int sdso_map_put(sdso_ctx* ctx, int frameID, int list, int n, const float* records) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, map_list_ok(list), "list other than 1 (active), 2 (marginalised) or 3 (out)");
  SDSO_REQUIRE(ctx, n >= 0 && (n == 0 || records), "negative n, or records missing");
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  MapList& L = map_state(ctx).kf[frameID].list[list - 1];
  SDSO_TRY(map_reserve(ctx, L, n, 0));
  if (n) {
    SDSO_HIP(ctx, hipMemcpyAsync(L.d, records, sizeof(float) * MAP_REC_FLOATS * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the array is the caller's again when the call returns
  }
  L.n = n;
  return SDSO_OK;
}

extern "C" int sdso_map_release_keyframe(sdso_ctx* ctx, int frameID) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->map) return SDSO_OK;
  auto it = ctx->map->kf.find(frameID);
  if (it == ctx->map->kf.end()) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));        // launches that read its lists may still be in flight
  ctx->map->kf.erase(it);
  return SDSO_OK;
}

extern "C" int sdso_map_clear(sdso_ctx* ctx) {
  if (!ctx) return SDSO_ERR_STATE;
  if (!ctx->map) return SDSO_OK;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->map->kf.clear();
  return SDSO_OK;
}

// ------------------------------------------------------------------ refreshPC
extern "C" int sdso_map_cloud(sdso_ctx* ctx, const sdso_map_cloud_t* C, float* xyz, uint8_t* rgb, int* first, int* kept) {
  if (!ctx) return SDSO_ERR_STATE;
  // ---- refusals.  Everything that can be judged without the device comes first; the bound then needs the counts of the named immature
  // groups, and a group whose sdso_imm_add_frame has not reported its count yet is waited for (that add, not the stream)
  SDSO_REQUIRE(ctx, C && first, "null sdso_map_cloud_t or first");
  SDSO_REQUIRE(ctx, C->n_frames >= 1 && C->n_frames <= MAP_MAX_FRAMES, "n_frames outside 1..8");
  SDSO_REQUIRE(ctx, C->frameID, "null frameID");
  SDSO_REQUIRE(ctx, C->scaledTH == C->scaledTH && C->absTH == C->absTH && C->minBS == C->minBS, "a threshold is NaN");
  const int nfr = C->n_frames;
  MapQuery Q;
  std::memset(&Q, 0, sizeof(Q));
  long long total = 0;
  int nwaves = 0;
  for (int k = 0; k < nfr; k++) {
    for (int j = 0; j < k; j++) SDSO_REQUIRE(ctx, C->frameID[j] != C->frameID[k], "a frame is named twice");
    SDSO_REQUIRE(ctx, map_find(ctx, C->frameID[k]), "unknown frameID");
  }
  for (int k = 0; k < nfr; k++) {
    const MapKeyframe* KF = map_find(ctx, C->frameID[k]);
    for (int st = 0; st < 4; st++) {
      MapCloudSeg& G = Q.seg[4 * k + st];
      G.status = st; G.frame = k; G.wbeg = nwaves;
      if (st == MAP_ST_IMMATURE) {
        if (C->imm_host_id && C->imm_host_id[k] >= 0) {
          SDSO_HIP(ctx, hipSetDevice(ctx->device));
          const int rc = imm_host_view(ctx, C->imm_host_id[k], &G.src, &G.n, &G.cap);   // (waits for the group's count, nothing else)
          SDSO_REQUIRE(ctx, G.src, "unknown immature group");
          if (rc) return rc;
        }
      } else {
        const MapList& L = KF->list[st - 1];
        G.src = L.d; G.n = L.n; G.cap = 0;
      }
      nwaves += (G.n + 63) / 64;
      total += G.n;
    }
  }
  SDSO_REQUIRE(ctx, total * MAP_PATTERN <= (long long)INT32_MAX, "more vertices than an int counts");
  SDSO_REQUIRE(ctx, C->cap >= 0 && (long long)C->cap >= total * MAP_PATTERN, "cap is below 8 x the sum of the list sizes");
  SDSO_REQUIRE(ctx, total == 0 || (xyz && rgb), "null xyz / rgb");
  Q.seg[4 * nfr].wbeg = nwaves;
  Q.nseg = 4 * nfr; Q.nwaves = nwaves;
  Q.K = map_calib(C->fx, C->fy, C->cx, C->cy);
  Q.scaledTH = C->scaledTH; Q.absTH = C->absTH; Q.minBS = C->minBS; Q.mode = C->mode;
  Q.world = C->camToWorld != nullptr;
  if (C->camToWorld) std::memcpy(Q.T, C->camToWorld, sizeof(float) * 12 * (size_t)nfr);
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  MapState& S = map_state(ctx);
  for (int k = 0; k <= nfr; k++) first[k] = 0;
  if (kept) std::memset(kept, 0, sizeof(int) * 4 * (size_t)nfr);
  if (!nwaves) { S.cloud_n = 0; return SDSO_OK; }
  // ---- one upload of the query, two kernels
  constexpr size_t kept_off = (sizeof(MapQuery) + 255) & ~(size_t)255, mask_off = kept_off + 256;
  static_assert(MAP_MAX_SEGS * sizeof(int) <= 256, "the per-list counters fit their block");
  const size_t work = mask_off + sizeof(unsigned long long) * (size_t)nwaves, out = (size_t)total * MAP_PATTERN * 3;
  SDSO_HIP(ctx, S.d_work.reserve(ctx->stream, work, work + work / 2 + 64));
  S.cloud_n = -1;
  SDSO_HIP(ctx, S.d_xyz.reserve(ctx->stream, out, out + out / 2 + 64));
  SDSO_HIP(ctx, S.d_rgb.reserve(ctx->stream, out, out + out / 2 + 64));
  char* stage = nullptr;
  SDSO_TRY(stage_reserve(ctx, S.stage, sizeof(MapQuery), &stage));
  std::memcpy(stage, &Q, sizeof(Q));
  SDSO_HIP(ctx, hipMemcpyAsync(S.d_work, stage, sizeof(MapQuery), hipMemcpyHostToDevice, ctx->stream));
  SDSO_TRY(stage_commit(ctx, S.stage));
  SDSO_HIP(ctx, hipMemsetAsync(S.d_work + kept_off, 0, 256, ctx->stream));
  const MapQuery* d_q = (const MapQuery*)S.d_work;
  int* d_kept = (int*)(S.d_work + kept_off);
  unsigned long long* d_mask = (unsigned long long*)(S.d_work + mask_off);
  const dim3 grid((nwaves + MAP_BLOCK / 64 - 1) / (MAP_BLOCK / 64));
  launch_timed(ctx, "k_map_mark", 2, k_map_mark, grid, dim3(MAP_BLOCK), d_q, d_kept, d_mask);
  launch_timed(ctx, "k_map_emit", 2, k_map_emit, grid, dim3(MAP_BLOCK), d_q, (const unsigned long long*)d_mask, S.d_xyz, S.d_rgb);
  SDSO_HIP(ctx, hipGetLastError());
  int seg_kept[MAP_MAX_SEGS];
  // SDSO_MAP_ONE_WAIT=1 (an A/B switch, sdso_internal.h): the counts and both arrays at their upper bound in one batch of copies behind
  // one wait, the used prefix handed on from pinned memory — what tools/time_map_cloud.py times against the default below
  if (dbg_env("SDSO_MAP_ONE_WAIT")) {
    const size_t nb = (size_t)total * MAP_PATTERN * 3, xyz_off = 256, rgb_off = xyz_off + sizeof(float) * nb;
    SDSO_TRY(ensure_pinned(ctx, rgb_off + nb));
    char* host = (char*)ctx->pinned;
    SDSO_HIP(ctx, hipMemcpyAsync(host, d_kept, sizeof(seg_kept), hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipMemcpyAsync(host + xyz_off, S.d_xyz, sizeof(float) * nb, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipMemcpyAsync(host + rgb_off, S.d_rgb, nb, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(seg_kept, host, sizeof(seg_kept));
    int pts = 0;
    for (int k = 0; k < nfr; k++) {
      first[k] = pts * MAP_PATTERN;
      for (int st = 0; st < 4; st++) { pts += seg_kept[4 * k + st]; if (kept) kept[4 * k + st] = seg_kept[4 * k + st]; }
    }
    first[nfr] = S.cloud_n = pts * MAP_PATTERN;
    if (pts) { std::memcpy(xyz, host + xyz_off, sizeof(float) * 3 * (size_t)S.cloud_n); std::memcpy(rgb, host + rgb_off, 3 * (size_t)S.cloud_n); }
    return SDSO_OK;
  }
  // ---- the counts, then the used prefix of the two arrays
  SDSO_HIP(ctx, hipMemcpyAsync(seg_kept, d_kept, sizeof(seg_kept), hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int pts = 0;
  for (int k = 0; k < nfr; k++) {
    first[k] = pts * MAP_PATTERN;
    for (int st = 0; st < 4; st++) { pts += seg_kept[4 * k + st]; if (kept) kept[4 * k + st] = seg_kept[4 * k + st]; }
  }
  first[nfr] = pts * MAP_PATTERN;
  S.cloud_n = pts * MAP_PATTERN;
  if (pts) {
    SDSO_HIP(ctx, hipMemcpyAsync(xyz, S.d_xyz, sizeof(float) * 3 * (size_t)S.cloud_n, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipMemcpyAsync(rgb, S.d_rgb, 3 * (size_t)S.cloud_n, hipMemcpyDeviceToHost, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SDSO_OK;
}

extern "C" int sdso_map_cloud_dev(sdso_ctx* ctx, void** xyz_dev, void** rgb_dev, int* n) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, xyz_dev && rgb_dev && n, "null argument");
  if (!ctx->map || ctx->map->cloud_n < 0) return sdso::fail(ctx, SDSO_ERR_STATE, "no sdso_map_cloud has run on this ctx");
  *xyz_dev = ctx->map->d_xyz; *rgb_dev = ctx->map->d_rgb; *n = ctx->map->cloud_n;
  return SDSO_OK;
}
