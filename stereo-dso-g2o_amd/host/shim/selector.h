#pragma once
#include "device.h"
namespace sdso_shim {
// PixelSelector (src/FullSystem/PixelSelector2.h): int makeMaps(const FrameHessian* fh, float* map_out, float density,
// int recursionsLeft = 1, bool plot = false, float thFactor = 1); currentPotential is the public member the callers reset.
class PixelSelector {
 public:
  explicit PixelSelector(Device& dev) : dev_(dev) {}
  int currentPotential = 3;
  int makeMaps(int frame_slot, float* map_out, float density, int recursionsLeft = 1, bool /*plot*/ = false, float thFactor = 1) {
    int n = 0;
    dev_.check(sdso_pixel_select(dev_.ctx(), frame_slot, density, recursionsLeft, thFactor, &currentPotential, map_out, &n), "sdso_pixel_select");
    return n;
  }

 private:
  Device& dev_;
};
// EnergyFunctional::marginalizeFrame's algebra (EnergyFunctional.cpp:554-660) on plain row-major arrays
inline void marginalizeFrame(int nFrames, int idx, const double* prior8, const double* delta_prior8, std::vector<double>& HM, std::vector<double>& bM) {
  const int m = 8 * (nFrames - 1) + 4;
  std::vector<double> Ho((size_t)m * m), bo(m);
  if (sdso_ba_marginalize_frame(nFrames, idx, prior8, delta_prior8, HM.data(), bM.data(), Ho.data(), bo.data()) != SDSO_OK)
    throw Error("sdso_ba_marginalize_frame: bad arguments");
  HM.swap(Ho); bM.swap(bo);
}
}  // namespace sdso_shim
