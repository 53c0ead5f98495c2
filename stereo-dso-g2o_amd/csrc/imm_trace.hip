// sdso_imm_trace: FullSystem::traceNewCoarseKey / traceNewCoarseNonKey (FullSystem.cpp:632-781) on the resident set.  traceOn runs in
// place (trace_on_point on a host's blob); the stereo chain of the non-key trace is launched with trace_pair_bind / launch_fresh_trace
// around this file's own prepare / back / accept kernels, and its points are written by fresh_point.
namespace sdso {
enum { IMM_C_FWD_GOOD = 6, IMM_C_STEREO_OUTLIER = 7, IMM_C_UPDATED = 8, IMM_C_UNREADABLE = 9 };   // counts[] of sdso_imm_trace past the histogram
// the named hosts of one sdso_imm_trace call, as kernel arguments (a few hundred bytes: nothing is copied to the device per call)
struct ImmTraceArgs {
  int nh, ntot;
  int off[SDSO_IMM_MAX_HOSTS + 1];   // first flat index of every host; flat index j = off[g] + i
  ImmHostDev H[SDSO_IMM_MAX_HOSTS];
  sdso_imm_geom_t G[SDSO_IMM_MAX_HOSTS];
};
struct ImmCalib { float Ki[9]; };
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
  float fu = kTraceParkedPixel, fv = kTraceParkedPixel, pm = 0.f, pM = NAN;   // a point that takes no trace is parked
  if (in && A.H[g].st[i] == IPS_GOOD) {
    const float tu = f[IMM_UV * N + (size_t)i * 2], tv = f[IMM_UV * N + (size_t)i * 2 + 1];
    if (trace_pattern_readable(tu, tv, w, h)) {
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
// The back point of forward point j (:691-697, and stereoMatch's :589-595): a fresh point of the other image at the forward trace's
// lastTraceUV.  good: the forward trace ran (skipF null: every point's did) and returned GOOD; run: its lastTraceUV addresses a readable
// pattern, and the back point takes its trace.  pmin / pmax null: the fresh interval 0 / NaN.
__device__ __forceinline__ void imm_back_point(int j, int w, int h, const TraceDev& F, const TraceDev& Bk, const uint8_t* __restrict__ skipF, uint8_t* __restrict__ skipB,
                                               const float* __restrict__ pmin, const float* __restrict__ pmax, bool& good, bool& run) {
  float bu = kTraceParkedPixel, bv = kTraceParkedPixel;
  good = !(skipF && skipF[j]) && F.lastTraceStatus[j] == IPS_GOOD;
  run = false;
  if (good) {
    const float tu = F.lastTraceUV[2 * j], tv = F.lastTraceUV[2 * j + 1];
    if (trace_pattern_readable(tu, tv, w, h)) { run = true; bu = tu; bv = tv; }
  }
  skipB[j] = run ? 0 : 1;
  fresh_point(Bk, j, bu, bv, 0.f, run && pmin ? pmin[j] : 0.f, run && pmax ? pmax[j] : NAN);
}
// :691-697: the back points at the forward trace's lastTraceUV, with the projected interval again
__global__ __launch_bounds__(256) void k_imm_back_points(int n, int w, int h, TraceDev F, TraceDev Bk, const uint8_t* __restrict__ skipF, uint8_t* __restrict__ skipB,
                                                         const float* __restrict__ pmin, const float* __restrict__ pmax, int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool good = false, run = false;
  if (j < n) imm_back_point(j, w, h, F, Bk, skipF, skipB, pmin, pmax, good, run);
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
  for (int s = 0; s < 6; s++) imm_count(counts, s, st == s);
}

extern "C" int sdso_imm_trace(sdso_ctx* ctx, int frame_slot, int right_slot, int ngeom, const sdso_imm_geom_t* geom, const float K[4], const float Ki[9],
                              float baseline, int* counts) {
  if (!ctx) return SDSO_ERR_STATE;
  SDSO_HIP(ctx, hipSetDevice(ctx->device));
  const bool nonkey = right_slot >= 0;
  SDSO_REQUIRE(ctx, ngeom >= 0 && ngeom <= SDSO_IMM_MAX_HOSTS && (ngeom == 0 || geom), "0 <= ngeom <= SDSO_IMM_MAX_HOSTS geometries");
  SDSO_REQUIRE(ctx, !nonkey || (K && Ki), "the non-key trace needs K and Ki");
  PyramidDev *PL = nullptr, *PR = nullptr;
  SDSO_TRY(frame_pyramid(ctx, frame_slot, &PL));
  const int w = PL->w[0], h = PL->h[0];
  if (nonkey) {
    SDSO_TRY(frame_pyramid_sized(ctx, right_slot, w, h, "the two frames differ in size", &PR, "unknown right frame slot"));
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
  A.nh = ngeom;
  SDSO_TRY(imm_host_table(ctx, hosts, ngeom, A.H, A.off, &A.ntot));
  for (int g = 0; g < SDSO_IMM_MAX_HOSTS; g++) A.G[g] = g < ngeom ? geom[g] : sdso_imm_geom_t();
  const int n = A.ntot;
  if (counts) for (int k = 0; k < SDSO_IMM_NCOUNTS; k++) counts[k] = 0;
  if (n == 0) return SDSO_OK;
  SDSO_HIP(ctx, S.d_counts.reserve(ctx->stream, SDSO_IMM_NCOUNTS, SDSO_IMM_NCOUNTS));
  SDSO_HIP(ctx, S.h_counts.reserve(ctx->stream, SDSO_IMM_NCOUNTS, SDSO_IMM_NCOUNTS));
  TraceDev base = TraceDev();   // traceOn takes its geometry from the point's host: the camera is the identity
  const float K0[4] = {1, 1, 0, 0};
  SDSO_TRY(trace_set_camera(ctx, base, *PL, K0, 0.f, 1));
  if (nonkey) {
    SDSO_TRY(trace_pair_bind(ctx, S.fwd, S.back, n, *PL, *PR, K, baseline, 1, 0));
  }
  SDSO_HIP(ctx, hipMemsetAsync(S.d_counts, 0, sizeof(int) * SDSO_IMM_NCOUNTS, ctx->stream));
  launch_timed(ctx, "k_imm_trace_on", 1, k_imm_trace_on, dim3((n + 3) / 4), dim3(256), A, base);
  if (nonkey) {
    const TraceDev& F = S.fwd.T;     // forward: points of the new left frame searched in the right one
    const TraceDev& Bk = S.back.T;   // back: points of the right frame searched in the left one
    uint8_t *skipF = S.fwd.skip(), *skipB = S.back.skip();
    float *pmin = S.fwd.pmin(), *pmax = S.fwd.pmax();
    ImmCalib C;
    for (int k = 0; k < 9; k++) C.Ki[k] = Ki[k];
    const dim3 g1((n + 255) / 256), b1(256);
    launch_timed(ctx, "k_imm_stereo_prepare", 2, k_imm_stereo_prepare, g1, b1, A, w, h, F, skipF, pmin, pmax, S.d_counts);
    launch_fresh_trace(ctx, F, *PL, skipF);
    launch_timed(ctx, "k_imm_back_points", 2, k_imm_back_points, g1, b1, n, w, h, F, Bk, (const uint8_t*)skipF, skipB, (const float*)pmin, (const float*)pmax, S.d_counts);
    launch_fresh_trace(ctx, Bk, *PR, skipB);
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
