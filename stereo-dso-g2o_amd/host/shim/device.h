#pragma once
#include <functional>   // (<functional>, <utility>, <vector>: for every part that includes this one)
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/sdso_abi.h"
namespace sdso_shim {
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
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
