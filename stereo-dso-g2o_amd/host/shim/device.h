#pragma once
#include <functional>   // (<functional>, <utility>, <vector>: for every part that includes this one)
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/sdso_abi.h"
namespace sdso_shim {
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
// One reference to an exported block of device buffers (sdso_shared): a frame's pyramid on its way from the tracking domain to the
// mapping domain (FullSystem.cpp:1203-1221), or a tracking template on its way back (:1102-1109).  Move-only; may be handed to
// another thread; the block lives while a slot of any Device or a Shared holds it.
class Shared {
 public:
  Shared() = default;
  explicit Shared(sdso_shared* h) : h_(h) {}
  ~Shared() { sdso_shared_release(h_); }
  Shared(Shared&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Shared& operator=(Shared&& o) noexcept {
    if (this != &o) { sdso_shared_release(h_); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  Shared(const Shared&) = delete;
  Shared& operator=(const Shared&) = delete;
  sdso_shared* get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  int holders() const { int n = 0; return sdso_shared_info(h_, nullptr, nullptr, &n) == SDSO_OK ? n : 0; }   // slots + handles

 private:
  sdso_shared* h_ = nullptr;
};
// A device buffer pool (sdso_pool): with one attached (Device::setPool), the level buffers of pyramids, their level-0 copies and the
// levels of tracking templates are parked when they leave a slot and handed out again behind stream waits — the hand-off of frames and
// templates between two Devices then makes no allocator call and no host wait in its steady state.  Move-only; this object is the
// caller's reference: the pool lives while it, an attached Device or a block exported under it does, so the order of destruction is free.
class Pool {
 public:
  Pool() = default;
  explicit Pool(int ordinal, size_t max_parked_bytes = (size_t)1 << 30) {
    if (sdso_pool_create(ordinal, max_parked_bytes, &p_) != SDSO_OK) throw Error("sdso_pool_create failed: no such HIP device");
  }
  ~Pool() { sdso_pool_release(p_); }
  Pool(Pool&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Pool& operator=(Pool&& o) noexcept {
    if (this != &o) { sdso_pool_release(p_); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  sdso_pool* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  sdso_pool_stats_t stats() const {
    sdso_pool_stats_t s{};
    if (sdso_pool_stats(p_, &s) != SDSO_OK) throw Error("sdso_pool_stats: no pool");
    return s;
  }
  // frees parked buffers whose work has completed until at most keep_bytes stay parked; no host wait
  void trim(size_t keep_bytes = 0) { if (sdso_pool_trim(p_, keep_bytes) != SDSO_OK) throw Error("sdso_pool_trim: no pool"); }

 private:
  sdso_pool* p_ = nullptr;
};
// One GPU + stream.  The reference serialises tracking under trackMutex and mapping under mapMutex;
// use one Device per such domain (or one shared Device and the same mutexes).
class Device {
 public:
  explicit Device(int ordinal = 0) {
    if (sdso_ctx_create(ordinal, &ctx_) != SDSO_OK) throw Error("sdso_ctx_create failed: no usable HIP device (there is no CPU fallback)");
  }
  ~Device() { sdso_ctx_destroy(ctx_); }
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;
  sdso_ctx* ctx() const { return ctx_; }
  void check(int rc, const char* what) const {
    if (rc != SDSO_OK) throw Error(std::string(what) + ": " + sdso_last_error(ctx_));
  }
  // FrameHessian::dIp mirrors: immutable after makeImages, so upload once per frame (key = shell->id / frameID)
  template <class FrameHessianT> void uploadFrame(int slot, const FrameHessianT* fh, int levels, const int* w, const int* h) {
    std::vector<const float*> p(levels);
    for (int l = 0; l < levels; l++) p[l] = reinterpret_cast<const float*>(fh->dIp[l]);  // Eigen::Vector3f is 3 packed floats
    check(sdso_upload_pyramid(ctx_, slot, levels, w, h, p.data()), "sdso_upload_pyramid");
  }
  void releaseFrame(int slot) { sdso_release_pyramid(ctx_, slot); }
  // deliverTrackedFrame (FullSystem.cpp:1203-1221) between two Devices on one GPU: the domain that built or ingested the pyramid exports
  // it, the other imports it under a slot of its own — no copy, no host wait, and the pyramid may still be on its way on the exporter's
  // stream.  From the export on the buffers are frozen: a later upload / ingest into either slot goes to fresh buffers.
  Shared exportFrame(int slot) {
    sdso_shared* h = nullptr;
    check(sdso_pyramid_export(ctx_, slot, &h), "sdso_pyramid_export");
    return Shared(h);
  }
  void importFrame(int slot, const Shared& s) { check(sdso_pyramid_import(ctx_, slot, s.get()), "sdso_pyramid_import"); }
  // From now on the level buffers of this Device's frames and templates come from and go to `pool` (of the same GPU; one pool serves
  // both Devices of the threaded binding); clearPool(): hipMalloc / hipFree, as without a pool.  On this Device's thread, at any time.
  void setPool(Pool& pool) { check(sdso_ctx_set_pool(ctx_, pool.get()), "sdso_ctx_set_pool"); }
  void clearPool() { check(sdso_ctx_set_pool(ctx_, nullptr), "sdso_ctx_set_pool"); }
  // Multi-GPU: one process per GPU; rank 0 makes the id (static uniqueId()), the caller ships the 128 bytes to the other ranks,
  // then every rank calls commInit (collective).  RCCL is resolved at run time; a missing librccl is an error, not a fallback.
  static void uniqueId(unsigned char id[128]) {
    if (sdso_comm_unique_id(id) != SDSO_OK) throw Error("sdso_comm_unique_id failed (librccl.so.1 not loadable?)");
  }
  void commInit(int nranks, int rank, const unsigned char id[128]) { check(sdso_comm_init(ctx_, nranks, rank, id), "sdso_comm_init"); }
  // traceStereo's sub-pixel refinement: false = DSO-native GN (ImmaturePoint.cpp:707-769), true = the fork's g2o GN on
  // EdgeTracePointUVDSO (ImmaturePoint.cpp:309-412)
  void setForkLiveTraceRefinement(bool on) { check(sdso_trace_set_gn_mode(ctx_, on ? 1 : 0), "sdso_trace_set_gn_mode"); }

 private:
  sdso_ctx* ctx_ = nullptr;
};
}  // namespace sdso_shim
