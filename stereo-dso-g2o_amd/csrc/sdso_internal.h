// Internal definitions of libsdso_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdint>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/sdso_abi.h"
#include "tile0_layout.h"
#include "share.h"
#include "devbuf.h"

namespace sdso {

// ---- constants of the reference (values @ file:line in SURVEY.md Appendix A)
#define SCALE_IDEPTH 1.0f
#define SCALE_XI_ROT 1.0f
#define SCALE_XI_TRANS 0.5f
#define SCALE_F 50.0f
#define SCALE_C 50.0f
#define SCALE_A 10.0f
#define SCALE_B 1000.0f
constexpr float kHuberTH = 9.0f;                 // settings.cpp:95
constexpr float kOutlierTHSumComponent = 2500.f; // settings.cpp:73

// The level buffers of an exported pyramid / template (share.h, share.hip): reference-counted, frozen, viewed by slots of any ctx on
// the device.  A slot whose `blk` is null owns its buffers alone, as every slot did before sdso_*_export existed.
struct HipShareBackend {   // share.h's backend
  typedef hipEvent_t Event;
  typedef hipStream_t Stream;
  int event_create(Event* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? 0 : 1; }
  void event_destroy(Event e) { hipEventDestroy(e); }
  int event_record(Event e, Stream s) { return hipEventRecord(e, s) == hipSuccess ? 0 : 1; }
  int event_wait(Event e) { return hipEventSynchronize(e) == hipSuccess ? 0 : 1; }
  int stream_wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess ? 0 : 1; }
  int stream_sync(Stream s) { return hipStreamSynchronize(s) == hipSuccess ? 0 : 1; }
  // non-blocking: 1 completed (pool.h).  "Not ready" is an answer, not an error: it must not be what a later hipGetLastError() after a
  // kernel launch on this thread reports.
  int event_query(Event e) {
    const hipError_t r = hipEventQuery(e);
    if (r == hipErrorNotReady) (void)hipGetLastError();
    return r == hipSuccess ? 1 : 0;
  }
  int alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? 0 : 1; }
  // the last holder may be a handle released on a thread whose current device is another one
  void free(void* p, int device) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != device) { hipSetDevice(device); hipFree(p); hipSetDevice(cur); }
    else hipFree(p);
  }
};
struct HipBufBackend {   // devbuf.h's backend
  typedef hipError_t Error;
  typedef hipStream_t Stream;
  Error dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  void dev_free(void* p) { hipFree(p); }
  Error host_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  void host_free(void* p) { hipHostFree(p); }
  Error stream_sync(Stream s) { return hipStreamSynchronize(s); }
};
// the work buffers a ctx owns alone (devbuf.h): device memory and pinned host memory
template <class T> using DevBuf = devbuf::Buf<HipBufBackend, T, devbuf::DEVICE>;
template <class T> using PinBuf = devbuf::Buf<HipBufBackend, T, devbuf::PINNED>;
typedef share::Block<HipShareBackend> ShareBlock;
typedef pool::Pool<HipShareBackend> DevPool;   // the device buffer pool (pool.h, pool.hip), attached by sdso_ctx_set_pool
// the slot gives up its view of `blk`; unsynced: work the ctx enqueued on it may still run on `stream` (an event is left in the block
// for whoever frees it), false after a stream synchronisation.  The last holder parks the buffers in the block's own pool, or else in
// `fallback` (the dropping ctx's pool), with no host wait; with neither it waits and frees, as ever.
void share_drop(ShareBlock* blk, hipStream_t stream, bool unsynced, DevPool* fallback = nullptr);

// A pyramid level on the device: one float4 {I, dx, dy, 0} per pixel (16-byte taps).
struct PyramidDev {
  int levels = 0;
  int w[SDSO_PYR_LEVELS] = {0}, h[SDSO_PYR_LEVELS] = {0};
  float4* d[SDSO_PYR_LEVELS] = {nullptr};
  ShareBlock* blk = nullptr;   // non-null: d[] are views into this exported block and must not be written (alloc_pyramid detaches first)
  // the two derived copies below are the ctx's own, built on its own stream, also where d[] is a view
  // level 0 once more as 12-byte pixels {I, dx, dy} in 5x2-pixel tiles (one 128-B line per tile, tile0_layout.h) for the BA
  // linearisation, built on first use
  char* tiled0 = nullptr;
  bool tiled_ok = false;
  // level-0 intensities alone (4 B per pixel) for the discrete epipolar search, which samples I only; built on first use
  float* plane0 = nullptr;
  bool plane_ok = false;
};
// pc_* of one reference keyframe: one float4 {u, v, idepth, color} per template point.
struct RefDev {
  int n[SDSO_PYR_LEVELS] = {0};
  float4* pc[SDSO_PYR_LEVELS] = {nullptr};
  int cap[SDSO_PYR_LEVELS] = {0};   // entries pc[l] was allocated for (>= n[l])
  ShareBlock* blk = nullptr;        // non-null: pc[] are views into this exported block and must not be written (ref_detach first)
  // everything below is the ctx's own and is never shared
  // A template built on the device without waiting for it (track_make_ref_dev): its counts are on their way into `counts_host`
  // (pinned) behind `counts_ev`; ref_counts() brings n[] up to date.  Every reader of n[] calls it first.
  bool counts_pending = false;
  int* counts_host = nullptr;
  hipEvent_t counts_ev = nullptr;
  // The level-0 map idepth[0] this template was built from, kept under sdso_track_keep_depth_map (coarse_depth.hip) for
  // sdso_track_depth_image (depth_image.hip).  One allocation, laid out by depth_map_layout: the map, the image call's 16-byte record and
  // its B3 image, so that any choice of outputs is one contiguous copy.  map_ok: the block holds the map of the template now installed.
  char* dmap = nullptr;
  int dmap_w = 0, dmap_h = 0;
  bool map_ok = false, image_ok = false;
};
// the kept block of a w x h map: [0, rec) the map (w*h floats) | [rec, rgb) {minID, maxID, allID.size(), circles} | [rgb, end) w*h*3 bytes
struct DepthMapLayout { size_t rec, rgb, end; };
inline DepthMapLayout depth_map_layout(int w, int h) {
  const size_t px = (size_t)w * h;
  return {sizeof(float) * px, sizeof(float) * px + 16, sizeof(float) * px + 16 + 3 * px};
}

struct ProfEntry {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // pending (start, stop) pairs
  double total_ms = 0;
  long launches = 0;
};

struct BaWindowDev;  // ba_window.hip
struct BaCtxState;   // ba_window.hip
struct TrackBatch;   // tracker_eval.hip
struct StereoState;  // stereo_batch.hip (a part of stereo.hip)
struct SelState;     // selector.hip
struct G2oState;     // g2o_factors.hip
struct DistMapState; // distmap.hip
struct IngestState;  // ingest.hip
struct ImmState;     // imm_set.hip (a part of stereo.hip)
struct InitState;    // init_stereo.hip (a part of stereo.hip)
struct Comm;         // comm.hip
struct RefWinState;  // ref_window.hip
struct BaDev;        // ba_kernels.h
struct MapState;     // map.hip

}  // namespace sdso

struct sdso_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::map<int, sdso::PyramidDev> pyr;
  std::map<int, sdso::RefDev> refs;
  std::map<int, sdso::BaWindowDev*> wins;
  // per-module state, owned by the ctx: null until the module's first call needs it, freed by the module's release_* (sdso_ctx_destroy)
  sdso::BaCtxState* ba = nullptr;       // staging, batch and resident GN loop of the BA
  sdso::TrackBatch* tb = nullptr;
  sdso::StereoState* stereo = nullptr;  // the prepared traceStereo batch and the matching batches
  sdso::SelState* sel = nullptr;        // the pixel selector's random pattern
  sdso::G2oState* g2o = nullptr;        // edge sets and partial systems of the g2o factors
  sdso::DistMapState* dm = nullptr;     // the level-1 CoarseDistanceMap
  sdso::IngestState* ingest = nullptr;  // calibration tables and raw-image staging of sdso_ingest_frame
  sdso::ImmState* imm = nullptr;        // the device-resident immature points, per host keyframe (sdso_imm_*)
  sdso::InitState* init = nullptr;      // the stereo initialiser: the Pnts of setFirstStereo and what STEP 3 reads of them (sdso_init_*)
  sdso::RefWinState* refwin = nullptr;  // STEP1 records of sdso_track_make_ref_from_window, per reference slot
  sdso::MapState* map = nullptr;        // the device-resident map: the point lists of every keyframe (sdso_map_*)
  std::shared_ptr<sdso::Comm> comm;     // shared with the contexts joined by sdso_comm_attach
  sdso::DevPool* pool = nullptr;        // sdso_ctx_set_pool (a reference of the ctx's own): where level buffers come from and go to; null: hipMalloc / hipFree
  // generic scratch
  sdso::DevBuf<void> scratch;
  // k_track_lm's cluster records: written by that kernel only, with tags that grow from call to call (no clearing between calls)
  sdso::DevBuf<void> lm_clusters;
  int lm_epoch = 0;
  sdso::PinBuf<void> pinned;
  int n_cu = 256;
  // CU partition (sdso_ctx_partition_cus): `stream` is masked to the large share of the CUs, `aux` to the small one; inside a batch's
  // resident GN loop the linearisation runs on `stream`, the Schur accumulation and the fused tail kernel on `aux` — next to the
  // linearisation of ANOTHER ctx's batch whose stream carries the same large mask.  aux == nullptr: no partition (everything on `stream`).
  hipStream_t aux = nullptr;
  hipEvent_t ev_main = nullptr, ev_aux = nullptr;
  int aux_cus = 0;
  int keep_depth_map = 0;   // sdso_track_keep_depth_map: templates built by track_make_ref_dev keep their level-0 map (RefDev::dmap)
  int gn_mode = 0;   // traceStereo refinement: 0 DSO-native, 1 fork-live g2o GN (sdso_trace_set_gn_mode)
  sdso::DevBuf<float> gammaB;   // device copy of CalibHessian::B (256 floats) for the gamma-weighted absSquaredGrad; null = identity response
  // device buffers of released BA windows, kept for the next upload (a window is re-uploaded for every keyframe)
  std::vector<std::pair<void*, size_t>> ba_pool;
  // optional in-library kernel timing (HIP events on ctx->stream), see sdso_prof_*
  int prof_on = 0;           // 0 off; 1 the dominant kernel of each workload; 2 every bracketed kernel (each bracket is two hipEventRecord on the
                             //   stream: ~5 us of queue time apiece, which a timed loop should not pay for kernels it does not report)
  std::map<std::string, sdso::ProfEntry> prof;
};

namespace sdso {

inline int fail(sdso_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define SDSO_HIP(ctx, expr)                                                                  \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return sdso::fail(ctx, SDSO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define SDSO_REQUIRE(ctx, cond, msg) \
  do {                               \
    if (!(cond)) return sdso::fail(ctx, SDSO_ERR_ARG, msg); \
  } while (0)

// a step that reports like its caller: anything but SDSO_OK ends the caller with that code (the step has set the ctx's error text)
#define SDSO_TRY(expr)          \
  do {                          \
    const int _rc = (expr);     \
    if (_rc) return _rc;        \
  } while (0)

int ensure_scratch(sdso_ctx* ctx, size_t bytes);
// ---- level buffers with or without a buffer pool (pool.hip).  Without one these are hipMalloc and `false`: the caller runs the code it
// always ran.
// `bytes` of device memory for a pyramid level or a level-0 copy (pool.h: EXACT), or at least `need` for a template level (ROUNDED;
// *got = what the buffer holds; without a pool: exactly `unpooled` bytes, the slack the call always allocated); from the pool the
// buffer comes ordered behind every earlier use on ctx->stream
hipError_t dev_acquire(sdso_ctx* ctx, void** p, size_t bytes);
hipError_t dev_acquire_rounded(sdso_ctx* ctx, void** p, size_t need, size_t unpooled, size_t* got);
// n buffers of one kind (pyramid levels and level-0 copies: pool::EXACT; template levels: pool::ROUNDED; null entries skipped) that this ctx alone used leave for its pool behind ONE event recorded on ctx->stream (none if
// `synced`: the caller has synchronised the stream); no host wait.  false: the ctx has no pool, nothing was done.
bool dev_park(sdso_ctx* ctx, pool::Match kind, int n, void* const* bufs, const size_t* bytes, bool synced);
inline size_t share_level_bytes(int kind, int dim0, int dim1) {   // a block's level buffer: w x h float4, or cap float4
  return sizeof(float4) * (kind == share::KIND_PYRAMID ? (size_t)dim0 * dim1 : (size_t)dim1);
}
// n[] of a reference whose template was enqueued without a synchronisation: waits for that template's counts only
inline int ref_counts(sdso_ctx* ctx, RefDev& R) {
  if (!R.counts_pending) return SDSO_OK;
  SDSO_HIP(ctx, hipEventSynchronize(R.counts_ev));
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) R.n[l] = R.counts_host[l] < R.cap[l] ? R.counts_host[l] : R.cap[l];   // (never past the allocation)
  R.counts_pending = false;
  return SDSO_OK;
}
// the levels of a template leave the slot: its own buffers are freed, a view drops its reference.  synced: the caller has synchronised
// the stream (always, without a pool); with a pool the buffers are parked, behind an event on the stream unless `synced`.
inline void ref_free_levels(sdso_ctx* ctx, RefDev& R, bool synced = true) {
  if (R.blk) { share_drop(R.blk, synced ? nullptr : ctx->stream, !synced, ctx->pool); R.blk = nullptr; }
  else {
    size_t bytes[SDSO_PYR_LEVELS];
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) bytes[l] = sizeof(float4) * (size_t)R.cap[l];
    if (!dev_park(ctx, pool::ROUNDED, SDSO_PYR_LEVELS, (void* const*)R.pc, bytes, synced))
      for (int l = 0; l < SDSO_PYR_LEVELS; l++) if (R.pc[l]) hipFree(R.pc[l]);
  }
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) { R.pc[l] = nullptr; R.n[l] = 0; R.cap[l] = 0; }
}
inline void ref_free(sdso_ctx* ctx, RefDev& R, bool synced = true) {
  ref_free_levels(ctx, R, synced);
  if (R.counts_host) hipHostFree(R.counts_host);
  if (R.counts_ev) hipEventDestroy(R.counts_ev);
  R.counts_host = nullptr; R.counts_ev = nullptr; R.counts_pending = false;
  if (R.dmap) hipFree(R.dmap);
  R.dmap = nullptr; R.dmap_w = R.dmap_h = 0; R.map_ok = R.image_ok = false;
}
// A writer is about to fill pc[] of a slot whose levels are a view: the slot leaves the frozen block to its other holders and starts
// from no buffers at all.  No host wait: what this ctx still runs on the block is covered by the event share_drop leaves in it.
inline void ref_detach(sdso_ctx* ctx, RefDev& R) {
  if (!R.blk) return;
  share_drop(R.blk, ctx->stream, true, ctx->pool);
  R.blk = nullptr;
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) { R.pc[l] = nullptr; R.n[l] = 0; R.cap[l] = 0; }
}
// ---- a frame slot as the entry points see it.  Every refusal is SDSO_ERR_ARG; nothing is launched or waited for before them.
// Level 0 and the sizes of the pyramid in `frame_slot`; `unknown` is the caller's refusal text where it names the slot.
inline int frame_pyramid(sdso_ctx* ctx, int frame_slot, PyramidDev** out, const char* unknown = "unknown frame slot") {
  auto ip = ctx->pyr.find(frame_slot);
  SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), unknown);
  *out = &ip->second;
  return SDSO_OK;
}
// the same for a slot whose level 0 must be w x h (the caller's w / h, or another frame's size), refused with the caller's text
inline int frame_pyramid_sized(sdso_ctx* ctx, int frame_slot, int w, int h, const char* differs, PyramidDev** out, const char* unknown = "unknown frame slot") {
  const int rc = frame_pyramid(ctx, frame_slot, out, unknown);
  if (rc) return rc;
  SDSO_REQUIRE(ctx, (*out)->w[0] == w && (*out)->h[0] == h, differs);
  return SDSO_OK;
}
// ---- what the tracker's entry points (tracker_*.hip, g2o_factors.hip) evaluate: one template level on one image level.  Every refusal
// is SDSO_ERR_ARG, or what ref_counts returns; nothing is launched before them.
// The image half: level `lvl` of the pyramid in `frame_slot`.  The kernels index the image with the caller's (w, h): they must be the
// uploaded level's size.
inline int track_image_level(sdso_ctx* ctx, int frame_slot, int lvl, int w, int h, const float4** img) {
  auto ip = ctx->pyr.find(frame_slot);
  SDSO_REQUIRE(ctx, ip != ctx->pyr.end(), "unknown frame slot");
  SDSO_REQUIRE(ctx, lvl >= 0 && lvl < ip->second.levels, "level not in the uploaded pyramid");
  SDSO_REQUIRE(ctx, w == ip->second.w[lvl] && h == ip->second.h[lvl], "w / h do not match the uploaded pyramid level");
  *img = ip->second.d[lvl];
  return SDSO_OK;
}
// Both halves.  The argument checks come before ref_counts (the four copies this replaces did not agree on the order): a call that is
// wrong in its arguments AND whose template's counts fail to arrive (SDSO_ERR_HIP) is refused with SDSO_ERR_ARG.
struct TrackLevel { const float4* pc; const float4* img; int n; };
inline int track_level(sdso_ctx* ctx, int ref_slot, int frame_slot, int lvl, int w, int h, TrackLevel* out) {
  auto ir = ctx->refs.find(ref_slot);
  SDSO_REQUIRE(ctx, ir != ctx->refs.end(), "unknown reference slot");
  int rc = track_image_level(ctx, frame_slot, lvl, w, h, &out->img);
  if (rc) return rc;
  rc = ref_counts(ctx, ir->second);
  if (rc) return rc;
  out->pc = ir->second.pc[lvl];
  out->n = ir->second.n[lvl];
  return SDSO_OK;
}
// what a trackNewestCoarse call reports before its first evaluation (CoarseTracker.cpp:846-850)
__host__ __device__ inline void track_result_reset(sdso_track_result_t& out) {
  for (int i = 0; i < 5; i++) { out.lastResiduals[i] = NAN; out.iterations[i] = 0; }
  for (int i = 0; i < 3; i++) out.lastFlowIndicators[i] = 1000;
  out.evaluations = 0; out.point_evals = 0; out.good = 0;
}
// the levels a trackNewestCoarse call may start from (the assert of CoarseTracker.cpp:853)
inline int track_coarsest_level_ok(sdso_ctx* ctx, const sdso_track_params_t& p) {
  SDSO_REQUIRE(ctx, p.coarsestLvl >= 0 && p.coarsestLvl < 5 && p.coarsestLvl < p.levels, "coarsestLvl out of range");
  return SDSO_OK;
}
// FullSystem::trackNewCoarse STEP2-4 (tracker_tries.hip) over the runner of a batch of tries: `runner` has track_newest_coarse_run's
// contract (tracker_lm_api.hip) — nhyp tries in one launch, in/out poses and affine pairs, results, event traces.  sdso_track_new_coarse
// passes the DSO-native runner, sdso_g2o_track_new_coarse (g2o_track_lm.hip) the fork-live one; refusals, records and phases are one text.
typedef int (*TrackBatchRunner)(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots, const sdso_track_params_t* prms,
                                sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* outs, sdso_track_trace_t* traces);
int track_new_coarse_with(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries, const sdso_se3_t* tries,
                          const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold, sdso_track_tries_result_t* out,
                          sdso_track_try_t* recs, TrackBatchRunner runner);
// Bracket the launches of one named kernel with HIP events when profiling is enabled.
// The A/B and diagnostic switches of the library (SDSO_BA_*, SDSO_TRK_*, SDSO_OPT_*, SDSO_PROF_BRACKET) exist only under SDSO_DEBUG_ENV=1,
// which is read ONCE per process: without it no environment variable changes what the library computes or launches, and no call reads
// the environment.  (tests/conftest.py sets the gate: the variant tests flip switches per call; bench.py does not.)
inline const char* dbg_env(const char* name) {
  static const bool on = [] { const char* g = getenv("SDSO_DEBUG_ENV"); return g && atoi(g) != 0; }();
  return on ? getenv(name) : nullptr;
}
struct ProfScope {
  sdso_ctx* ctx;
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  ProfScope(sdso_ctx* c, const char* n, int level = 1) : ctx(c), name(n) {
    if (ctx->prof_on < level) return;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a, ctx->stream);
  }
  ~ProfScope() {
    if (!a) return;
    hipEventRecord(b, ctx->stream);
    ctx->prof[name].ev.emplace_back(a, b);
  }
};
// ONE kernel launch, timed exactly when profiling is enabled: hipExtLaunchKernelGGL ties the two events to the start and the end of
// the dispatch itself (the timestamps rocprofv3 reports), where a pair of hipEventRecord calls around the launch also counts the
// dispatch latency after the first record (≈ 10 us on a 390-us kernel: bench.py's figure sat 2.5 % above rocprofv3's).
// SDSO_PROF_BRACKET=1: the old record / launch / record bracket.
// The arguments convert to the kernel's parameter types P, as in a plain call (a DevBuf names its pointer).
template <typename... P, typename... A>
inline void launch_timed(sdso_ctx* ctx, const char* name, int level, void (*kernel)(P...), const dim3& grid, const dim3& block, const A&... args) {
  static const bool bracket = dbg_env("SDSO_PROF_BRACKET") != nullptr;
  if (ctx->prof_on >= level && !bracket) {
    hipEvent_t ea = nullptr, eb = nullptr;
    hipEventCreate(&ea); hipEventCreate(&eb);
    hipExtLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ea, eb, 0, static_cast<P>(args)...);
    ctx->prof[name].ev.emplace_back(ea, eb);
    return;
  }
  ProfScope ps(ctx, name, level);
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, static_cast<P>(args)...);
}
int ensure_pinned(sdso_ctx* ctx, size_t bytes);
// Pinned host staging for the enqueue-only entry points (window uploads and table refreshes of the BA, raw images of the frame ingest),
// grown on demand.  Two buffers taken in turn, each with an event that marks the last copy enqueued from it (stage_commit): a caller that
// commits need not synchronise the stream — the buffer is only waited for when its turn comes again, two reservations later.  A caller
// that does not commit synchronises the stream itself before the same StageBuf is reserved again.
struct StageBuf { char* p[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0}; hipEvent_t ev[2] = {nullptr, nullptr}; bool busy[2] = {false, false}; int cur = 0; };
inline int stage_reserve(sdso_ctx* ctx, StageBuf& b, size_t bytes, char** out) {
  b.cur ^= 1;
  const int k = b.cur;
  if (b.busy[k]) { SDSO_HIP(ctx, hipEventSynchronize(b.ev[k])); b.busy[k] = false; }
  if (bytes > b.cap[k]) {
    if (b.p[k]) { SDSO_HIP(ctx, hipStreamSynchronize(ctx->stream)); hipHostFree(b.p[k]); }
    b.p[k] = nullptr; b.cap[k] = 0;
    const size_t want = (bytes * 3 / 2 + 4095) & ~(size_t)4095;
    SDSO_HIP(ctx, hipHostMalloc((void**)&b.p[k], want));
    b.cap[k] = want;
  }
  *out = b.p[k];
  return SDSO_OK;
}
inline int stage_commit(sdso_ctx* ctx, StageBuf& b) {   // everything that reads the latest reservation has been enqueued on ctx->stream
  const int k = b.cur;
  if (!b.ev[k]) SDSO_HIP(ctx, hipEventCreateWithFlags(&b.ev[k], hipEventDisableTiming));
  SDSO_HIP(ctx, hipEventRecord(b.ev[k], ctx->stream));
  b.busy[k] = true;
  return SDSO_OK;
}
inline void stage_free(StageBuf& b) {
  for (int k = 0; k < 2; k++) { if (b.ev[k]) hipEventDestroy(b.ev[k]); if (b.p[k]) hipHostFree(b.p[k]); }
  b = StageBuf();
}
// the device copy of the map the latest sdso_pixel_select of this ctx made, if it was made on `frame_slot` at w x h; *num = the
// number of its non-zero entries (selector.hip)
void selector_forget_slot(sdso_ctx* ctx, int frame_slot);   // the slot is released or takes another image: that map is no longer its map
bool selector_final_map(sdso_ctx* ctx, int frame_slot, int w, int h, const float** map, int* num);
int ensure_tiled0(sdso_ctx* ctx, PyramidDev& P);   // ctx.hip
int ensure_plane0(sdso_ctx* ctx, PyramidDev& P);   // ctx.hip
int pyramid_prepare(sdso_ctx* ctx, int frame_slot, int w, int h, PyramidDev** out);   // ctx.hip
int pyramid_finish_levels(sdso_ctx* ctx, PyramidDev& P);                              // ctx.hip

// ---- the pieces sdso_track_make_ref_from_window (ref_window.hip) chains on the device
// where the L->R->L chain of sdso_stereo_match_batch leaves its results (device pointers into the ctx's match batches)
struct MatchChainOut { const float *idepth_stereo, *idepth_min, *idepth_max, *fwd_uv, *back_uv; const uint8_t *status_fwd, *status_back; };
int stereo_match_chain_dev(sdso_ctx* ctx, int slot_a, int slot_b, const float K[4], float baseline, int mode_right_first, int n,
                           const float* const in[6], const uint8_t* skip_fwd, MatchChainOut* out);                            // stereo_match.hip
int track_make_ref_dev(sdso_ctx* ctx, int ref_slot, int frame_slot, int n, const int* d_u, const int* d_v, const float* d_idp, const float* d_wgt,
                       int* pc_n_out, bool sync_end);                                                                         // coarse_depth.hip
// what a BA window offers a reader of its post-state (ba_api.hip): SDSO_ERR_ARG for an unknown window, SDSO_ERR_STATE unless an optimize
// call has ended on it and nothing has edited it since, it is outside a batch and none of its residuals is linearised
struct BaRefView { const BaDev* dev; int nf, np, nr, w, h, last_frame_slot; float K[4]; };
int ba_ref_view(sdso_ctx* ctx, int win, BaRefView* out);
// the frames of a window as the map keys them (map.hip): frameID of every frame, and the points of host h: [host_pt_beg[h], host_pt_beg[h + 1])
int ba_window_hosts(sdso_ctx* ctx, int win, int frameID[8], int host_pt_beg[9]);
// the current blob of an immature group (imm_layout.h) with its count resolved; *f = nullptr without such a group (imm_set.hip)
int imm_host_view(sdso_ctx* ctx, int host_id, const float** f, int* n, int* cap);
// the latest sdso_imm_activate of the ctx (imm_activate.hip): its n records in toOptimize order, on the host (pinned; the integer members
// are what a caller may read there) and on the device in the set's own buffer; consumed: imm_activation_consumed has been called since
struct ImmActRec;   // imm_layout.h
struct ImmActView { bool valid = false, consumed = false; int nf = 0, n = 0, w = 0, h = 0; const ImmActRec* h_rec = nullptr; const ImmActRec* d_rec = nullptr; };
void imm_activation_view(sdso_ctx* ctx, ImmActView* out);
void imm_activation_consumed(sdso_ctx* ctx);
// the points of a window where they lie (ba_api.hip): p_geo = {u, v, idepth, idepth_zero} and the host frame of every point, in the
// window's order.  SDSO_ERR_ARG for an unknown window.
struct BaPointsView { const float4* p_geo; const int* p_host; int nf, np, w, h; };
int ba_window_points(sdso_ctx* ctx, int win, BaPointsView* out);

// ------------------------------------------------------------------ device helpers
// getInterpolatedElement33 (src/util/globalFuncs.h:73-86) on the float4 image.
// Same operation order as the reference so that per-point results are bit-identical to the CPU.
__device__ __forceinline__ float3 interp33(const float4* __restrict__ img, float x, float y, int width) {
  const int ix = (int)x;
  const int iy = (int)y;
  const float dx = x - ix;
  const float dy = y - iy;
  const float dxdy = dx * dy;
  const float4* bp = img + ix + iy * width;
  const float4 p00 = bp[0], p10 = bp[1], p01 = bp[width], p11 = bp[1 + width];
  const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
  float3 r;
  r.x = w11 * p11.x + w01 * p01.x + w10 * p10.x + w00 * p00.x;
  r.y = w11 * p11.y + w01 * p01.y + w10 * p10.y + w00 * p00.y;
  r.z = w11 * p11.z + w01 * p01.z + w10 * p10.z + w00 * p00.z;
  return r;
}
// getInterpolatedElement31 (globalFuncs.h:122-135)
__device__ __forceinline__ float interp31(const float4* __restrict__ img, float x, float y, int width) {
  const int ix = (int)x;
  const int iy = (int)y;
  const float dx = x - ix;
  const float dy = y - iy;
  const float dxdy = dx * dy;
  const float4* bp = img + ix + iy * width;
  return dxdy * bp[1 + width].x + (dy - dxdy) * bp[width].x + (dx - dxdy) * bp[1].x + (1 - dx - dy + dxdy) * bp[0].x;
}

// getInterpolatedElement31 on the intensity plane (same expression, a quarter of the bytes per tap)
__device__ __forceinline__ float interp31_plane(const float* __restrict__ I, float x, float y, int width) {
  const int ix = (int)x;
  const int iy = (int)y;
  const float dx = x - ix;
  const float dy = y - iy;
  const float dxdy = dx * dy;
  const float* bp = I + ix + iy * width;
  return dxdy * bp[1 + width] + (dy - dxdy) * bp[width] + (dx - dxdy) * bp[1] + (1 - dx - dy + dxdy) * bp[0];
}

// value of a compile-time-constant lane in every lane (v_readlane_b32: scalar broadcast, no LDS crossbar trip)
__device__ __forceinline__ float lane_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int lane_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// 64-lane butterfly sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}


// Sum N (multiple of 4) per-lane values over the 64 lanes of a wave with gfx950's half/row swaps instead of one
// 6-step butterfly per value: v_permlane32_swap exchanges the upper half of one register with the lower half of
// another, so one swap + one add finishes the 32-lane step for TWO values; v_permlane16_swap does the same for the
// 16-lane rows.  N values -> N/4 registers, each then folded inside its rows by four DPP row rotations:
// 2.5 instructions per value instead of 12.  emit(k, sum) is called by one lane per value.
template <int N, class Emit>
__device__ __forceinline__ void wave_reduce_rows(const float* v, Emit emit) {
  static_assert(N % 4 == 0, "N must be a multiple of 4");
  const int lane = threadIdx.x & 63;
  float z[N / 4];
#pragma unroll
  for (int m = 0; m < N / 4; m++) {
    float x[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[4 * m + 2 * h]), __float_as_uint(v[4 * m + 2 * h + 1]), false, false);
      x[h] = __uint_as_float(r[0]) + __uint_as_float(r[1]);   // rows 0,1: v[4m+2h] (32-lane partials), rows 2,3: v[4m+2h+1]
    }
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x[0]), __float_as_uint(x[1]), false, false);
    float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);  // rows: v[4m], v[4m+2], v[4m+1], v[4m+3] (16-lane partials)
    t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x128, 0xf, 0xf, false));   // row_ror:8
    t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x124, 0xf, 0xf, false));   // row_ror:4
    t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x122, 0xf, 0xf, false));   // row_ror:2
    t += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(t), 0x121, 0xf, 0xf, false));   // row_ror:1
    z[m] = t;
  }
  if ((lane & 15) == 0) {
    const int row = lane >> 4;
    const int sub = row == 0 ? 0 : row == 1 ? 2 : row == 2 ? 1 : 3;
#pragma unroll
    for (int m = 0; m < N / 4; m++) emit(4 * m + sub, z[m]);
  }
}

}  // namespace sdso
