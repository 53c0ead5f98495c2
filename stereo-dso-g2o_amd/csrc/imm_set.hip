// The device-resident immature points of a ctx (sdso_imm_*): the set itself.  FullSystem::makeNewTraces (FullSystem.cpp:1600-1629) and
// STEP 5 of activatePointsMT (:948-957) on arrays that never leave the device; imm_trace.hip and imm_activate.hip work on the set in place,
// imm_match.hip reads it.
//
// Layout: one blob of kImmFloats * cap floats and cap status bytes per host, its members as imm_layout.h states them.  Every host has a
// second blob of the same size: a removal gathers into it and the two swap (imm_swap_blobs).
namespace sdso {

struct ImmHostDev { float* f; uint8_t* st; int n, cap; };
struct ImmHost {
  int w = 0, h = 0, cap = 0;
  int n = -1;                       // -1: the count of the add that made this host has not been read yet (h_n is valid after ev)
  DevBuf<float> f[2];               // [0] current, [1] the target of the next removal gather
  DevBuf<uint8_t> st[2];
  DevBuf<int> d_n;
  PinBuf<int> h_n;
  hipEvent_t ev = nullptr;
};
// the results of the latest sdso_imm_stereo_match (imm_match.hip), in buffers no other call writes: counts | idepth | accepted | status_fwd |
// status_back on the device with a pinned mirror, and the dense map of the latest call that built one
struct ImmMatchKept {
  DevBuf<char> d;
  PinBuf<char> h;                   // its first `have` bytes hold the device's
  int cap = 0;                      // points both buffers hold
  bool valid = false;
  int n = 0;
  size_t have = 0;
  DevBuf<float> d_map;
  bool map_valid = false, map_latest = false;   // a map is kept; the latest call built it
  int map_w = 0, map_h = 0;
};
struct ImmState {
  std::map<int, ImmHost> hosts;
  ImmMatchKept match;
  TraceBatch fwd, back;             // the stereo chain of the non-key trace, over the concatenated points of the named hosts
  DevBuf<int> d_counts;             // SDSO_IMM_NCOUNTS
  PinBuf<int> h_counts;
  StageBuf stage;                   // selection maps, removal orders and sdso_imm_activate's tables on their way to the device
  // the results of the latest sdso_imm_activate: header | decisions | records (pinned), for sdso_imm_activate_fetch
  PinBuf<char> h_act;
  bool act_valid = false;
  int act_nf = 0, act_ntot = 0, act_nsel = 0;
  // the same records once more on the device, in a buffer no other call writes, for sdso_ba_window_update_activated: act_nsel entries of
  // ImmActRec (imm_layout.h); the w x h of that call; consumed: an update has taken them into a window (cleared by every sdso_imm_activate)
  DevBuf<char> d_act;
  int act_w = 0, act_h = 0;
  bool act_consumed = false;
};
static ImmState& imm_state(sdso_ctx* ctx) { if (!ctx->imm) ctx->imm = new ImmState(); return *ctx->imm; }
static void imm_free_host(ImmHost& H) {   // (the stream is idle, or has never seen the host)
  if (H.ev) hipEventDestroy(H.ev);
  H = ImmHost();
}
// a fresh host for `cap` points: a group (devbuf.h); nothing but buffers is left behind when this fails
static int imm_alloc_host(sdso_ctx* ctx, ImmHost& H, int cap) {
  const size_t C = (size_t)cap;
  H.cap = 0;
  for (int k = 0; k < 2; k++) {
    SDSO_HIP(ctx, H.f[k].reserve(ctx->stream, kImmFloats * C, kImmFloats * C));
    SDSO_HIP(ctx, H.st[k].reserve(ctx->stream, C, C));
  }
  SDSO_HIP(ctx, H.d_n.reserve(ctx->stream, 1, 1));
  SDSO_HIP(ctx, H.h_n.reserve(ctx->stream, 1, 1));
  SDSO_HIP(ctx, hipEventCreateWithFlags(&H.ev, hipEventDisableTiming));
  H.cap = cap;
  return SDSO_OK;
}
void release_immature(sdso_ctx* ctx) {
  ImmState* S = ctx->imm;
  if (!S) return;
  for (auto& kv : S->hosts) if (kv.second.ev) hipEventDestroy(kv.second.ev);
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
// host `host_id` of the set with its count resolved; *out = nullptr without one (no set, or no such host), which the caller judges
static int imm_find_resolved(sdso_ctx* ctx, int host_id, ImmHost** out) {
  *out = nullptr;
  if (!ctx->imm) return SDSO_OK;
  auto it = ctx->imm->hosts.find(host_id);
  if (it == ctx->imm->hosts.end()) return SDSO_OK;
  *out = &it->second;
  return imm_resolve(ctx, it->second);
}
int imm_host_view(sdso_ctx* ctx, int host_id, const float** f, int* n, int* cap) {
  ImmHost* H = nullptr;
  *f = nullptr; *n = 0; *cap = 0;
  const int rc = imm_find_resolved(ctx, host_id, &H);
  if (H) { *f = H->f[0]; *n = rc ? 0 : H->n; *cap = H->cap; }
  return rc;
}
// after a gather into the second blob has been enqueued: that blob is the host's current one
static void imm_swap_blobs(ImmHost& H) { std::swap(H.f[0], H.f[1]); std::swap(H.st[0], H.st[1]); }

// ---- the named hosts of one call as its kernels see them (a few hundred bytes of kernel arguments: nothing is copied to the device per
// call): H[g], and the flat index j = off[g] + i over their points, off[nh] = *ntot.  A null hosts[g] is a group without points (n = 0);
// the entries from nh on are empty.  Waits for the counts of the named hosts, so the caller checks its arguments first.
static int imm_host_table(sdso_ctx* ctx, ImmHost* const hosts[], int nh, ImmHostDev H[SDSO_IMM_MAX_HOSTS], int off[SDSO_IMM_MAX_HOSTS + 1], int* ntot) {
  off[0] = 0;
  for (int g = 0; g < SDSO_IMM_MAX_HOSTS; g++) {
    H[g] = ImmHostDev{nullptr, nullptr, 0, 0};
    if (g < nh && hosts[g]) {
      SDSO_TRY(imm_resolve(ctx, *hosts[g]));
      H[g] = ImmHostDev{hosts[g]->f[0], hosts[g]->st[0], hosts[g]->n, hosts[g]->cap};
    }
    off[g + 1] = off[g] + H[g].n;
  }
  *ntot = off[nh];
  return SDSO_OK;
}
template <class Args>
__device__ __forceinline__ int imm_host_of(const Args& A, int j) {
  int g = 0;
  while (g + 1 < A.nh && j >= A.off[g + 1]) g++;
  return g;
}

// the sdso_trace_points_t array of every member, in the order of imm_member(); null: my_type, which that struct does not have
static float* sdso_trace_points_t::*const kImmField[kImmMembers] = {
    &sdso_trace_points_t::u_stereo, &sdso_trace_points_t::v_stereo, nullptr, &sdso_trace_points_t::idepth_min_stereo, &sdso_trace_points_t::idepth_max_stereo,
    &sdso_trace_points_t::quality, &sdso_trace_points_t::color, &sdso_trace_points_t::weights, &sdso_trace_points_t::gradH, &sdso_trace_points_t::energyTH,
    &sdso_trace_points_t::lastTraceUV, &sdso_trace_points_t::lastTracePixelInterval};

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

// ---- sdso_imm_add_frame's two compactions (imm_compact.hip): the map's candidates in raster order (L = w, one segment per row), then
// the candidates the constructor kept
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

// STEP 5 on the device: float c (c == kImmFloats: the status byte) of entry j of the new arrays is that of entry i of the old ones
__device__ __forceinline__ void imm_gather_one(int j, int i, int c, const float* __restrict__ f, const uint8_t* __restrict__ st, float* __restrict__ fo,
                                               uint8_t* __restrict__ sto, int cap) {
  if (c == kImmFloats) { sto[j] = st[i]; return; }
  const ImmMember M = imm_member_of_float(c);
  const int o = M.off, wd = M.width;
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
  PyramidDev* pyr = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &pyr));
  const int w = pyr->w[0], h = pyr->h[0];
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
  SDSO_TRY(ensure_scratch(ctx, bytes));
  float* q = (float*)ctx->scratch;
  if (selection_map) {
    char* stage = nullptr;
    SDSO_TRY(stage_reserve(ctx, S.stage, sizeof(float) * npx, &stage));
    std::copy(selection_map, selection_map + npx, (float*)stage);
    SDSO_HIP(ctx, hipMemcpyAsync(q, stage, sizeof(float) * npx, hipMemcpyHostToDevice, ctx->stream));
    SDSO_TRY(stage_commit(ctx, S.stage));
    d_map = q; q += npx;
  }
  const size_t C = (size_t)cap;
  float *cu = q, *cv = q + C, *ct = q + 2 * C, *cc = q + 3 * C, *cw = q + 11 * C, *cg = q + 19 * C, *ce = q + 23 * C;
  int* d_row = (int*)(q + 24 * C);
  int* d_seg = d_row + h;
  int* d_ncand = d_seg + nseg2;

  ImmHost H;
  H.w = w; H.h = h;
  int rc = imm_alloc_host(ctx, H, cap);
  if (rc) return rc;

  auto enqueue = [&]() -> int {
    const int one = 0x41000000;   // 8.0f: candidates past the count (the selector's bound) sit on a harmless pixel for the constructor kernel
    SDSO_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)cu, one, 2 * C, ctx->stream));
    const ImmMapPred mp{d_map, w, h};
    const ImmMapEmit me{d_map, w, cap, cu, cv, ct};
    launch_timed(ctx, "k_imm_map_count", 2, k_imm_segcount<ImmMapPred>, dim3(h), dim3(256), mp, (int)npx, w, d_row);
    launch_timed(ctx, "k_imm_scan", 2, k_imm_scan, dim3(1), dim3(256), d_row, h, d_ncand);
    launch_timed(ctx, "k_imm_map_write", 2, (k_imm_segwrite<ImmMapPred, ImmMapEmit>), dim3(h), dim3(256), mp, me, (int)npx, w, (const int*)d_row);
    launch_timed(ctx, "k_immature_init", 2, k_immature_init, dim3(nseg2), dim3(256), (const float4*)pyr->d[0], w, cap, (const float*)cu, (const float*)cv, cc, cw, cg, ce);
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
  R = std::move(H);
  if (n_out) {
    SDSO_TRY(imm_resolve(ctx, R));
    *n_out = R.n;
  }
  return SDSO_OK;
}

extern "C" int sdso_imm_count(sdso_ctx* ctx, int host_id, int* n) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_REQUIRE(ctx, n, "null argument");
  *n = 0;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  ImmHost* H = nullptr;
  SDSO_TRY(imm_find_resolved(ctx, host_id, &H));
  if (H) *n = H->n;
  return SDSO_OK;
}

extern "C" int sdso_imm_get(sdso_ctx* ctx, int host_id, sdso_trace_points_t* out, float* my_type) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  SDSO_REQUIRE(ctx, out, "null argument");
  ImmHost* Hp = nullptr;
  const int rc = imm_find_resolved(ctx, host_id, &Hp);
  SDSO_REQUIRE(ctx, Hp, "unknown host_id");
  if (rc) return rc;
  ImmHost& H = *Hp;
  const int n = out->n = H.n;
  if (n == 0) return SDSO_OK;
  for (int m = 0; m < kImmMembers; m++) {
    float* dst = kImmField[m] ? out->*kImmField[m] : my_type;
    const ImmMember M = imm_member(m);
    if (dst) SDSO_HIP(ctx, hipMemcpyAsync(dst, H.f[0] + M.off * (size_t)H.cap, sizeof(float) * (size_t)M.width * n, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out->lastTraceStatus) SDSO_HIP(ctx, hipMemcpyAsync(out->lastTraceStatus, H.st[0], n, hipMemcpyDeviceToHost, ctx->stream));
  SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SDSO_OK;
}

extern "C" int sdso_imm_remove_order(int n, const uint8_t* flags, int* n_out, int* src) {
  if (n < 0 || !n_out || (n && (!flags || !src))) return SDSO_ERR_ARG;
  *n_out = imm_remove_order(n, flags, src);
  return SDSO_OK;
}

extern "C" int sdso_imm_remove(sdso_ctx* ctx, int host_id, int n, const uint8_t* flags) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  ImmHost* Hp = nullptr;
  int rc = imm_find_resolved(ctx, host_id, &Hp);
  SDSO_REQUIRE(ctx, Hp, "unknown host_id");
  if (rc) return rc;
  ImmHost& H = *Hp;
  ImmState& S = *ctx->imm;
  SDSO_REQUIRE(ctx, n == H.n && (n == 0 || flags), "n differs from the host's count");
  if (n == 0) return SDSO_OK;
  char* stage = nullptr;
  SDSO_TRY(stage_reserve(ctx, S.stage, sizeof(int) * (size_t)n, &stage));
  int n_new = 0;
  rc = sdso_imm_remove_order(n, flags, &n_new, (int*)stage);
  if (rc) return sdso::fail(ctx, rc, "sdso_imm_remove_order");
  if (n_new == n) return SDSO_OK;   // nothing flagged: the order does not change
  H.n = n_new;
  if (n_new == 0) return SDSO_OK;
  SDSO_TRY(ensure_scratch(ctx, sizeof(int) * (size_t)n_new));
  int* d_src = (int*)ctx->scratch;
  SDSO_HIP(ctx, hipMemcpyAsync(d_src, stage, sizeof(int) * (size_t)n_new, hipMemcpyHostToDevice, ctx->stream));
  SDSO_TRY(stage_commit(ctx, S.stage));
  const int threads = n_new * (kImmFloats + 1);
  launch_timed(ctx, "k_imm_gather", 2, k_imm_gather, dim3((threads + 255) / 256), dim3(256), n_new, (const int*)d_src, (const float*)H.f[0], (const uint8_t*)H.st[0], H.f[1],
               H.st[1], H.cap);
  SDSO_HIP(ctx, hipGetLastError());
  imm_swap_blobs(H);
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
  H.w = w; H.h = h; H.n = n;
  int rc = imm_alloc_host(ctx, H, std::max(n, 1));
  if (rc) return rc;
  auto copy = [&]() -> int {
    for (int m = 0; m < kImmMembers; m++) {
      const float* src = kImmField[m] ? P->*kImmField[m] : my_type;
      const ImmMember M = imm_member(m);
      SDSO_HIP(ctx, hipMemcpyAsync(H.f[0] + M.off * (size_t)H.cap, src, sizeof(float) * (size_t)M.width * n, hipMemcpyHostToDevice, ctx->stream));
    }
    SDSO_HIP(ctx, hipMemcpyAsync(H.st[0], P->lastTraceStatus, n, hipMemcpyHostToDevice, ctx->stream));
    SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the arrays are the caller's again when the call returns
    return SDSO_OK;
  };
  if (n) {
    rc = copy();
    if (rc) { hipStreamSynchronize(ctx->stream); imm_free_host(H); return rc; }
  }
  S.hosts[host_id] = std::move(H);
  return SDSO_OK;
}
