// The device buffer pool on HIP: pool.h's bookkeeping behind sdso_pool_*, and the two calls through which the level buffers of pyramids
// and templates come and go (dev_acquire*, dev_park).  No kernel in here and no hipMallocAsync: the ordering rule is pool.h's own text —
// a parked buffer carries the events of its earlier uses, the taker's stream waits for them, and nothing is freed before they completed.
#include "sdso_internal.h"
#include "pool.h"

struct sdso_pool { sdso::DevPool* core; };   // one reference (the caller's) to the pool

namespace sdso {

hipError_t dev_acquire(sdso_ctx* ctx, void** p, size_t bytes) {
  if (!ctx->pool) return hipMalloc(p, bytes);
  HipShareBackend be;
  size_t got = 0;
  return ctx->pool->acquire(be, bytes, pool::EXACT, ctx->stream, p, &got) ? hipErrorOutOfMemory : hipSuccess;
}

hipError_t dev_acquire_rounded(sdso_ctx* ctx, void** p, size_t need, size_t unpooled, size_t* got) {
  if (!ctx->pool) { *got = unpooled; return hipMalloc(p, unpooled); }
  HipShareBackend be;
  return ctx->pool->acquire(be, need, pool::ROUNDED, ctx->stream, p, got) ? hipErrorOutOfMemory : hipSuccess;
}

bool dev_park(sdso_ctx* ctx, pool::Match kind, int n, void* const* bufs, const size_t* bytes, bool synced) {
  if (!ctx->pool) return false;
  bool any = false;
  for (int i = 0; i < n; i++) any = any || bufs[i];
  if (!any) return true;
  HipShareBackend be;
  std::vector<hipEvent_t> ev;
  if (!synced) {
    hipEvent_t e = nullptr;
    if (be.event_create(&e) == 0 && be.event_record(e, ctx->stream) == 0) ev.push_back(e);
    else {   // no event to park them behind: today's wait
      if (e) be.event_destroy(e);
      be.stream_sync(ctx->stream);
      ctx->pool->count_host_wait();
    }
  }
  ctx->pool->park(be, kind, n, bufs, bytes, std::move(ev));
  return true;
}

void release_pool(sdso_ctx* ctx) {   // sdso_ctx_destroy, after every slot has parked what it held
  if (!ctx->pool) return;
  HipShareBackend be;
  ctx->pool->release(be);
  ctx->pool = nullptr;
}

}  // namespace sdso

using namespace sdso;

extern "C" int sdso_pool_create(int device_ordinal, size_t max_parked_bytes, sdso_pool** out) {
  if (!out) return SDSO_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SDSO_ERR_NODEV;
  if (device_ordinal < 0 || device_ordinal >= ndev) return SDSO_ERR_NODEV;
  *out = new sdso_pool{new DevPool(device_ordinal, max_parked_bytes)};
  return SDSO_OK;
}

extern "C" int sdso_ctx_set_pool(sdso_ctx* ctx, sdso_pool* pool) {
  if (!ctx) return SDSO_ERR_ARG;
  SDSO_REQUIRE(ctx, !pool || pool->core, "released pool");
  SDSO_REQUIRE(ctx, !pool || pool->core->device() == ctx->device, "the pool belongs to another device (a pool serves the ctxs of one device)");
  DevPool* next = pool ? pool->core : nullptr;
  if (next == ctx->pool) return SDSO_OK;
  if (next) next->retain();
  // what the ctx holds stays where it is: buffers are parked by byte size whoever allocated them, and freed by hipFree without a pool
  release_pool(ctx);
  ctx->pool = next;
  return SDSO_OK;
}

extern "C" int sdso_pool_stats(const sdso_pool* pool, sdso_pool_stats_t* out) {
  if (!pool || !pool->core || !out) return SDSO_ERR_ARG;
  const auto s = pool->core->stats();
  out->hits = s.hits; out->misses = s.misses; out->frees = s.frees; out->host_waits = s.host_waits; out->overflow_waits = s.overflow_waits;
  out->parked_buffers = s.parked_buffers; out->parked_bytes = s.parked_bytes;
  return SDSO_OK;
}

extern "C" int sdso_pool_trim(sdso_pool* pool, size_t keep_bytes) {
  if (!pool || !pool->core) return SDSO_ERR_ARG;
  HipShareBackend be;
  pool->core->trim(be, keep_bytes);
  return SDSO_OK;
}

extern "C" void sdso_pool_release(sdso_pool* pool) {
  if (!pool) return;
  HipShareBackend be;
  if (pool->core) pool->core->release(be);
  delete pool;
}
