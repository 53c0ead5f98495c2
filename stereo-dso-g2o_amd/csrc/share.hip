// Frames and tracking templates handed between contexts, device to device: share.h's bookkeeping on HIP, and the export / import calls.
// FullSystem::deliverTrackedFrame queues fh / fh_right for mappingLoop (FullSystem.cpp:1203-1221); the tracking thread swaps in the
// template makeKeyFrame built (FullSystem.cpp:1102-1109).  No kernel in here: ownership, ordering between streams, lifetimes.
#include "sdso_internal.h"
#include "share.h"

namespace sdso {

void share_drop(ShareBlock* blk, hipStream_t stream, bool unsynced, DevPool* fallback) {
  HipShareBackend be;
  share::drop_pooled(be, blk, stream, unsynced, fallback, share_level_bytes);   // (share::drop itself where there is no pool)
}

void release_g2o_ref(sdso_ctx* ctx, int ref_slot);     // g2o_factors.hip
void refwin_forget_slot(sdso_ctx* ctx, int ref_slot);  // ref_window.hip

}  // namespace sdso

using namespace sdso;

struct sdso_shared { ShareBlock* blk; };

namespace {

// the block of buffers a slot of `src` owns so far; under a pool the block names it and holds a reference to it
ShareBlock* adopt_slot(sdso_ctx* src, int kind, int levels, void* const* bufs, const int* dim0, const int* dim1) {
  ShareBlock* b = share::adopt<HipShareBackend>(kind, src->device, levels, bufs, dim0, dim1);
  if (src->pool) { b->pool = src->pool; b->pool->retain(); }
  return b;
}

// one more holder (the handle) behind everything `src` has enqueued; a block made for this export goes again if it fails
int export_common(sdso_ctx* src, ShareBlock** slot_blk, ShareBlock* b, sdso_shared** out) {
  HipShareBackend be;
  if (share::export_ref<HipShareBackend>(be, b, src->stream)) {
    if (!*slot_blk) { if (b->pool) b->pool->release(be); delete b; }   // (the buffers stay the slot's own)
    return sdso::fail(src, SDSO_ERR_HIP, "recording the export's ready event failed");
  }
  *slot_blk = b;
  *out = new sdso_shared{b};
  return SDSO_OK;
}

int import_checks(sdso_ctx* dst, const sdso_shared* h, int kind) {
  SDSO_REQUIRE(dst, h && h->blk, "null handle");
  SDSO_REQUIRE(dst, h->blk->kind == kind, kind == share::KIND_PYRAMID ? "the handle is a tracking template, not a pyramid" : "the handle is a pyramid, not a tracking template");
  SDSO_REQUIRE(dst, h->blk->device == dst->device, "the block lives on another device (peer copies are out of scope: replicate the frame)");
  return SDSO_OK;
}

}  // namespace

extern "C" int sdso_pyramid_export(sdso_ctx* src, int frame_slot, sdso_shared** out) {
  if (!src) return SDSO_ERR_ARG;
  SDSO_REQUIRE(src, out, "null argument");
  *out = nullptr;
  PyramidDev* P = nullptr;
  SDSO_TRY(frame_pyramid(src, frame_slot, &P));
  SDSO_HIP(src, hipSetDevice(src->device));
  ShareBlock* b = P->blk;
  if (!b) b = adopt_slot(src, share::KIND_PYRAMID, P->levels, (void* const*)P->d, P->w, P->h);
  return export_common(src, &P->blk, b, out);
}

extern "C" int sdso_pyramid_import(sdso_ctx* dst, int frame_slot, sdso_shared* h) {
  if (!dst) return SDSO_ERR_ARG;
  SDSO_TRY(import_checks(dst, h, share::KIND_PYRAMID));
  SDSO_HIP(dst, hipSetDevice(dst->device));
  ShareBlock* b = h->blk;
  PyramidDev N;
  auto it = dst->pyr.find(frame_slot);
  if (it != dst->pyr.end()) {
    PyramidDev& O = it->second;
    selector_forget_slot(dst, frame_slot);
    if (O.blk && O.w[0] == b->dim0[0] && O.h[0] == b->dim1[0]) {
      // a view of the same size goes: no host wait, and the ctx's own derived buffers stay for the new image
      share_drop(O.blk, dst->stream, true, dst->pool);   // (the last holder under a pool parks the levels: no free, no wait)
      N.tiled0 = O.tiled0; N.plane0 = O.plane0;
      dst->pyr.erase(it);
    } else {
      SDSO_TRY(sdso_release_pyramid(dst, frame_slot));   // buffers of the slot's own are freed behind a wait, as ever
    }
  }
  HipShareBackend be;
  if (share::import_ref<HipShareBackend>(be, b, dst->stream)) {
    void* own[2] = {N.tiled0, N.plane0};
    const size_t own_bytes[2] = {tile0_bytes(b->dim0[0], b->dim1[0]), sizeof(float) * (size_t)b->dim0[0] * b->dim1[0]};
    if ((N.tiled0 || N.plane0) && !dev_park(dst, pool::EXACT, 2, own, own_bytes, false)) { hipStreamSynchronize(dst->stream); hipFree(N.tiled0); hipFree(N.plane0); }
    return sdso::fail(dst, SDSO_ERR_HIP, "hipStreamWaitEvent on the block's ready event failed");
  }
  N.levels = b->levels;
  for (int l = 0; l < b->levels; l++) { N.w[l] = b->dim0[l]; N.h[l] = b->dim1[l]; N.d[l] = (float4*)b->buf[l]; }
  N.blk = b;
  dst->pyr[frame_slot] = N;
  return SDSO_OK;
}

extern "C" int sdso_track_export_ref(sdso_ctx* src, int ref_slot, sdso_shared** out) {
  if (!src) return SDSO_ERR_ARG;
  SDSO_REQUIRE(src, out, "null argument");
  *out = nullptr;
  auto ir = src->refs.find(ref_slot);
  SDSO_REQUIRE(src, ir != src->refs.end(), "unknown reference slot");
  SDSO_HIP(src, hipSetDevice(src->device));
  RefDev& R = ir->second;
  SDSO_TRY(ref_counts(src, R));   // the block carries final counts: a wait for this template's counts only
  ShareBlock* b = R.blk;
  if (!b) b = adopt_slot(src, share::KIND_TEMPLATE, SDSO_PYR_LEVELS, (void* const*)R.pc, R.n, R.cap);
  return export_common(src, &R.blk, b, out);
}

extern "C" int sdso_track_import_ref(sdso_ctx* dst, int ref_slot, sdso_shared* h) {
  if (!dst) return SDSO_ERR_ARG;
  SDSO_TRY(import_checks(dst, h, share::KIND_TEMPLATE));
  SDSO_HIP(dst, hipSetDevice(dst->device));
  ShareBlock* b = h->blk;
  RefDev& R = dst->refs[ref_slot];
  bool own = false;
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) own = own || (!R.blk && R.pc[l]);
  if (own && dst->pool && !dst->g2o) {
    ref_free_levels(dst, R, false);   // under a pool the slot's own levels are parked behind an event: no host wait
  } else if (own || dst->g2o) {   // buffers of the slot's own (or edge sets built on its template) are freed behind a wait, as ever
    SDSO_HIP(dst, hipStreamSynchronize(dst->stream));
    release_g2o_ref(dst, ref_slot);
    ref_free_levels(dst, R);
  } else {
    ref_detach(dst, R);    // a view goes with no host wait
  }
  R.counts_pending = false;           // (a template of the slot's own whose counts were on their way is gone)
  R.map_ok = R.image_ok = false;      // the kept level-0 map and the STEP1 records are the builder's, not the block's
  refwin_forget_slot(dst, ref_slot);
  HipShareBackend be;
  if (share::import_ref<HipShareBackend>(be, b, dst->stream)) return sdso::fail(dst, SDSO_ERR_HIP, "hipStreamWaitEvent on the block's ready event failed");
  for (int l = 0; l < SDSO_PYR_LEVELS; l++) { R.pc[l] = (float4*)b->buf[l]; R.n[l] = b->dim0[l]; R.cap[l] = b->dim1[l]; }
  R.blk = b;
  return SDSO_OK;
}

extern "C" int sdso_shared_info(const sdso_shared* h, int* kind, int* device, int* holders) {
  if (!h || !h->blk) return SDSO_ERR_ARG;
  if (kind) *kind = h->blk->kind;
  if (device) *device = h->blk->device;
  if (holders) *holders = h->blk->holders.load(std::memory_order_acquire);
  return SDSO_OK;
}

extern "C" void sdso_shared_release(sdso_shared* h) {
  if (!h) return;
  share_drop(h->blk, nullptr, false);   // a handle enqueues nothing
  delete h;
}

extern "C" int sdso_shared_debug_buffers(sdso_ctx* ctx, int kind, int slot, unsigned long long* ptrs, int* is_view) {
  if (!ctx) return SDSO_ERR_ARG;
  SDSO_REQUIRE(ctx, ptrs, "null argument");
  SDSO_REQUIRE(ctx, kind == share::KIND_PYRAMID || kind == share::KIND_TEMPLATE, "kind is 0 (pyramid) or 1 (template)");
  if (kind == share::KIND_PYRAMID) {
    PyramidDev* P = nullptr;
    SDSO_TRY(frame_pyramid(ctx, slot, &P));
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) ptrs[l] = (unsigned long long)(uintptr_t)P->d[l];
    if (is_view) *is_view = P->blk != nullptr;
  } else {
    auto ir = ctx->refs.find(slot);
    SDSO_REQUIRE(ctx, ir != ctx->refs.end(), "unknown reference slot");
    for (int l = 0; l < SDSO_PYR_LEVELS; l++) ptrs[l] = (unsigned long long)(uintptr_t)ir->second.pc[l];
    if (is_view) *is_view = ir->second.blk != nullptr;
  }
  return SDSO_OK;
}
