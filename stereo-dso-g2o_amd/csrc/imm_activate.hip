// ------------------------------------------------------------------ activatePointsMT STEP 2-5 on the set (FullSystem.cpp:837-957)
// sdso_imm_activate enqueues, without a host round trip in between:
//   k_imm_act_classify   the gates of STEP 2 per candidate, read from the groups' blobs (dm_classify, shared with k_select_classify)
//   k_distmap_select     the order-dependent rest of STEP 2 (distmap.hip, unchanged)
//   segcount/scan/write  the SELECTed candidates in order = toOptimize
//   k_imm_activate       optimizeImmaturePoint per entry of that list, one wave per point (activate_point of activate.hip, shared with
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
// (one entry of toOptimize: ImmActRec, imm_layout.h)
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
  const int g = blockIdx.x, t = threadIdx.x;
  const int n = A.H[g].n, base = A.off[g];
  const int per = (n + 255) / 256;
  const int b = min(n, t * per), e = min(n, b + per);
  int sum = 0;
  for (int k = b; k < e; k++) sum += flag[base + k];
  int run = block_exclusive_scan(sum, &hdr[ACT_H_FLAGGED + g]);
  for (int k = b; k < e; k++) { pref[base + k] = run; run += flag[base + k]; }
}
// The loop of STEP 5 in closed form (imm_layout.h: imm_back_slot, imm_final_src; test_imm_layout.cpp holds it against the loop itself).
// back[k] = the k-th survivor from the back, for the survivors at indices >= m.
__global__ __launch_bounds__(256) void k_imm_act_back(ImmActArgs A, const uint8_t* __restrict__ flag, const int* __restrict__ pref, const int* __restrict__ hdr,
                                                      int* __restrict__ back) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j), i = j - A.off[g];
  const int n = A.H[g].n, nflag = hdr[ACT_H_FLAGGED + g], m = n - nflag;
  if (flag[j] || i < m) return;
  back[A.off[g] + imm_back_slot(n, nflag, i, pref[j])] = i;
}
// src[j] (i < m) = the old index of the entry that ends at index i: itself, or for the k-th hole the k-th survivor from the back
__global__ __launch_bounds__(256) void k_imm_act_src(ImmActArgs A, const uint8_t* __restrict__ flag, const int* __restrict__ pref, const int* __restrict__ hdr,
                                                     const int* __restrict__ back, int* __restrict__ src) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.ntot) return;
  const int g = imm_host_of(A, j), i = j - A.off[g];
  const int m = A.H[g].n - hdr[ACT_H_FLAGGED + g];
  if (i >= m) return;
  src[j] = imm_final_src(i, flag[j] != 0, pref[j], back + A.off[g]);
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
    PyramidDev* pyr = nullptr;
    SDSO_TRY(frame_pyramid_sized(ctx, P->frame_slot[f], P->w, P->h, "pyramid size differs from w/h", &pyr));
    imgs[f] = pyr->d[0];
    auto it = S.hosts.find(P->host_id[f]);
    if (it == S.hosts.end()) continue;
    SDSO_REQUIRE(ctx, it->second.w == P->w && it->second.h == P->h, "the group's frame differs in size from w/h");
    hosts[f] = &it->second;
  }
  ImmActArgs A;
  ImmActOut O;
  A.nf = nf; A.nh = nh;
  int rc = imm_host_table(ctx, hosts, nh, A.H, A.off, &A.ntot);   // a walked frame without a group has no candidates
  if (rc) return rc;
  for (int g = 0; g < SDSO_IMM_MAX_HOSTS; g++) {
    const bool walked = g < nh, group = walked && hosts[g];
    A.G[g] = walked ? P->geom[g] : sdso_distmap_geom_t(); A.flagged[g] = walked ? P->host_flagged[g] : 0;
    O.f[g] = group ? hosts[g]->f[1] : nullptr; O.st[g] = group ? hosts[g]->st[1] : nullptr;
  }
  const int n = A.ntot;
  if (hosts[nh]) SDSO_TRY(imm_resolve(ctx, *hosts[nh]));

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
  SDSO_TRY(ensure_scratch(ctx, bytes));
  S.act_valid = false;                                    // from here on the previous activation's records (h_act, d_act) may be freed or overwritten
  SDSO_HIP(ctx, S.h_act.reserve(ctx->stream, res_bytes, (res_bytes * 3 / 2 + 4095) & ~(size_t)4095));
  // the records' own buffer (below): the scratch is the next call's to overwrite
  SDSO_HIP(ctx, S.d_act.reserve(ctx->stream, sizeof(ImmActRec) * N, (sizeof(ImmActRec) * N * 3 / 2 + 4095) & ~(size_t)4095));
  char* dp = (char*)ctx->scratch;
  int* d_hdr = (int*)(dp + o_hdr);
  uint8_t* d_dec = (uint8_t*)(dp + o_dec);
  int* h_hdr = (int*)S.h_act;
  for (int k = 0; k < ACT_H_INTS; k++) h_hdr[k] = 0;
  if (n) {
    char* stage = nullptr;
    SDSO_TRY(stage_reserve(ctx, S.stage, tab_bytes, &stage));
    float* tf = (float*)stage;
    std::copy(P->pair_R, P->pair_R + (size_t)nf * nf * 9, tf);
    std::copy(P->pair_t, P->pair_t + (size_t)nf * nf * 3, tf + (size_t)nf * nf * 9);
    std::copy(P->pair_aff, P->pair_aff + (size_t)nf * nf * 2, tf + (size_t)nf * nf * 12);
    std::copy(imgs, imgs + SDSO_IMM_MAX_HOSTS, (const float4**)(stage + (o_img - o_tab)));
    SDSO_HIP(ctx, hipMemcpyAsync(dp + o_tab, stage, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    SDSO_TRY(stage_commit(ctx, S.stage));
    SDSO_HIP(ctx, hipMemsetAsync(d_hdr, 0, sizeof(int) * ACT_H_INTS, ctx->stream));
    uint8_t* d_flag = (uint8_t*)(dp + o_flag);
    int *d_iu = (int*)(dp + o_iu), *d_iv = (int*)(dp + o_iv), *d_list = (int*)(dp + o_list), *d_pref = (int*)(dp + o_pref), *d_back = (int*)(dp + o_back),
        *d_src = (int*)(dp + o_src), *d_seg = (int*)(dp + o_seg);
    float *d_frac = (float*)(dp + o_frac), *d_thr = (float*)(dp + o_thr);
    ImmActRec* d_rec = (ImmActRec*)(dp + o_rec);
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_act_classify", 2, k_imm_act_classify, g1, b1, A, P->currentMinActDist, P->minTraceQuality, w1, h1, d_dec, d_flag, d_iu, d_iv, d_frac, d_thr,
                 d_hdr);
    SDSO_TRY(dm_run_select(ctx, n, d_dec, d_iu, d_iv, d_frac, d_thr, 0, d_hdr + ACT_H_NSEL));
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
    // the records outlive the scratch: device to device into the set's own buffer, enqueued behind the chain (nothing waits for it here;
    // sdso_ba_window_update_activated reads them on this stream)
    if (nsel) SDSO_HIP(ctx, hipMemcpyAsync(S.d_act, dp + o_rec, sizeof(ImmActRec) * nsel, hipMemcpyDeviceToDevice, ctx->stream));
    for (int g = 0; g < nh; g++) {
      const int nflag = h_hdr[ACT_H_FLAGGED + g];
      if (!hosts[g] || nflag == 0) continue;
      hosts[g]->n -= nflag;
      imm_swap_blobs(*hosts[g]);
    }
  }
  S.act_valid = true; S.act_nf = nf; S.act_ntot = n; S.act_nsel = h_hdr[ACT_H_NLIST];
  S.act_w = P->w; S.act_h = P->h; S.act_consumed = false;
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

namespace sdso {
void imm_activation_view(sdso_ctx* ctx, ImmActView* out) {
  *out = ImmActView();
  if (!ctx->imm || !ctx->imm->act_valid) return;
  const ImmState& S = *ctx->imm;
  const size_t o_rec = sizeof(int) * ACT_H_INTS + (((size_t)S.act_ntot + 15) & ~(size_t)15);   // header | decisions | records, as sdso_imm_activate lays them out
  out->valid = true; out->consumed = S.act_consumed;
  out->nf = S.act_nf; out->n = S.act_nsel; out->w = S.act_w; out->h = S.act_h;
  out->h_rec = (const ImmActRec*)(S.h_act + o_rec); out->d_rec = (const ImmActRec*)S.d_act;
}
void imm_activation_consumed(sdso_ctx* ctx) { if (ctx->imm) ctx->imm->act_consumed = true; }
}  // namespace sdso
