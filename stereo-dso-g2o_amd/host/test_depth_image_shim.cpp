// sdso_shim::CoarseTracker::debugPlotIDepthMap / debugPlotIDepthMapFloat on stand-ins for the reference's types.
// tests/test_depth_image_shim_gpu.py writes a window as raw arrays (the files of test_tracking_ref_shim) and runs
//   test_depth_image_shim <dir> frame      optimize, setCoarseTrackingRef(ba, frameHessians, fh_right), then the two members twice with a
//                                          recording wrapper: the first call with *minID_pt = *maxID_pt = -1, the second against the first's range
//   test_depth_image_shim <dir> onelevel   the same tracker told of a one-level frame (w[1] == 0): both members return before any push
// and compares what the wrapper received (out_<mode>_*.bin) with the C-ABI's results on the same window.
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

// ---- util/MinimalImage.h:32-57, :118-122: the two images the members make, and IOWrapper/Output3DWrapper.h:160, :170
struct Vec3b { unsigned char v[3]; };
template <class T> struct OwningImage {
  int w, h; T* data; bool ownData;
  OwningImage(int w_, int h_) : w(w_), h(h_), data(new T[(size_t)w_ * h_]), ownData(true) {}
  OwningImage(int w_, int h_, T* data_) : w(w_), h(h_), data(data_), ownData(false) {}
  OwningImage(const OwningImage&) = delete;
  ~OwningImage() { if (ownData) delete[] data; }
};
using MinimalImageB3 = OwningImage<Vec3b>;
using MinimalImageF = OwningImage<float>;
struct Output3DWrapper {                                  // records every push
  std::vector<std::vector<unsigned char>> b3;
  std::vector<std::vector<float>> f;
  std::vector<const float*> f_data;
  std::vector<FrameHessian*> kf;
  int w = 0, h = 0;
  void pushDepthImage(MinimalImageB3* image) {
    w = image->w; h = image->h;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(image->data);
    b3.emplace_back(p, p + (size_t)3 * w * h);
  }
  void pushDepthImageFloat(MinimalImageF* image, FrameHessian* KF) {
    f.emplace_back(image->data, image->data + (size_t)image->w * image->h);
    f_data.push_back(image->data);
    kf.push_back(KF);
  }
};

using Tracker = sdso_shim::CoarseTracker<SE3, AffLight, Mat33, Vec3>;

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: test_depth_image_shim <dir> frame|onelevel\n"); return 2; }
  const std::string dir = argv[1], mode = argv[2];
  const bool onelevel = mode == "onelevel";
  if (!onelevel && mode != "frame") { std::fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
  try {
    sdso_shim::Device dev(0);
    const auto m = load<int>(dir, "meta");                         // nf np nr w h its solverMode levels swapA swapB
    const int levels = m[7];
    WindowGraph G;
    WindowGraph::Options opt;
    opt.levels = levels; opt.frames_on_file = m[0] + 1;            // frame nf on file: the right image of the newest keyframe
    opt.last_state_from_file = true; opt.point_hessians = true; opt.swap_a = m[8]; opt.swap_b = m[9];
    G.build(dir, opt);
    const int nf = G.nf, w = G.w, h = G.h;
    std::vector<int> wv(levels), hv(levels);
    for (int l = 0; l < levels; l++) { wv[l] = w >> l; hv[l] = h >> l; }
    for (FrameHessian* fh : G.fhs) dev.uploadFrame(fh->slot, fh, levels, wv.data(), hv.data());
    auto slot_of_fh = [](FrameHessian* fh) { return fh->slot; };

    sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, 0);
    ba.writeBackProjections = false;
    ba.upload(&G.ef, &G.HC, w, h, /*solverMode=*/G.meta[6], 1e12, 1e8, true, slot_of_fh);
    ba.optimize(G.meta[5], &G.ef, &G.HC);

    std::vector<FrameHessian*> frameHessians(G.fhs.begin(), G.fhs.begin() + nf);
    Output3DWrapper rec, rec2;
    std::vector<Output3DWrapper*> wraps = {&rec, &rec2};
    Tracker trk(dev, /*ref_slot=*/1, /*publishDepthImages=*/!wraps.empty());
    trk.slot_of = [](const void* fh) { return static_cast<const FrameHessian*>(fh)->slot; };
    trk.baseline = (float)G.calib[8];
    trk.makeK(&G.HC, onelevel ? 1 : levels, w, h);                 // one level: w[1] stays 0, as CoarseTracker's constructor leaves it
    trk.setCoarseTrackingRef(ba, frameHessians, G.fhs[nf]);

    float minID = -1, maxID = -1;
    std::vector<float> ranges;
    std::vector<int> counts;
    for (int call = 0; call < 2; call++) {
      trk.debugPlotIDepthMap<MinimalImageB3>(&minID, &maxID, wraps);
      trk.debugPlotIDepthMapFloat<MinimalImageF, FrameHessian>(wraps);
      ranges.push_back(minID); ranges.push_back(maxID);
      counts.push_back(trk.depthImageCounts[0]); counts.push_back(trk.depthImageCounts[1]);
    }
    // null range pointers: the new range, nothing written back
    trk.debugPlotIDepthMap<MinimalImageB3>(nullptr, &maxID, wraps);
    ranges.push_back(minID); ranges.push_back(maxID);

    const int pushes = (int)rec.b3.size(), fpushes = (int)rec.f.size();
    bool same = rec2.b3.size() == rec.b3.size() && rec2.f.size() == rec.f.size();
    for (size_t i = 0; same && i < rec.b3.size(); i++) same = rec.b3[i] == rec2.b3[i];
    bool kf_ok = true, wrapped = true;
    for (FrameHessian* k : rec.kf) kf_ok = kf_ok && k == frameHessians.back();
    for (size_t i = 0; i < rec.f_data.size(); i++) wrapped = wrapped && rec.f_data[i] == rec2.f_data[i];   // no copy between the wrappers
    std::vector<int> info = {pushes, fpushes, same ? 1 : 0, kf_ok ? 1 : 0, wrapped ? 1 : 0, rec.w, rec.h};
    dump(dir, mode + "_info", info);
    dump(dir, mode + "_ranges", ranges);
    dump(dir, mode + "_counts", counts);
    for (int i = 0; i < pushes; i++) dump(dir, mode + "_b3_" + std::to_string(i), rec.b3[i]);
    for (int i = 0; i < fpushes; i++) dump(dir, mode + "_f_" + std::to_string(i), rec.f[i]);
    std::printf("%s: %d B3 pushes, %d float pushes, range %.9g %.9g\n", mode.c_str(), pushes, fpushes, minID, maxID);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_depth_image_shim: %s\n", e.what());
    return 1;
  }
  return 0;
}
