// Driver for sdso_shim::ImmaturePoints::stereoMatch on stand-in types that carry the reference's member names (Eigen, Sophus and OpenCV
// are not available here).  tests/test_stereo_match_shim_gpu.py writes the inputs as raw arrays, runs this program and compares what it
// dumps with the C-ABI path.
//   test_stereo_match_shim run <dir>
// meta = w h levels; calib = fx fy cx cy baseline density; left_dI<l> = the pyramid of the left image; right = level 0 of the right one.
// The body of FullSystem::stereoMatch (FullSystem.cpp:549-629) after makeImages: makeNewTraces, stereoMatch, release where the reference
// deletes fh.  Dumped: the idepth map (w*h*3 floats, rows packed) and `counter`; printed: counter, the points of the group before and
// after release.
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

// cv::Mat as stereoMatch uses it (CV_32FC3): data and step.  The rows carry padding, as a cv::Mat's may.
struct Mat {
  int rows, cols;
  size_t step;
  std::vector<unsigned char> store;
  unsigned char* data;
  Mat(int rows_, int cols_) : rows(rows_), cols(cols_), step((size_t)cols_ * 3 * sizeof(float) + 16), store((size_t)rows_ * step, 0), data(store.data()) {}
};

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");
  const int w = meta[0], h = meta[1], levels = meta[2];
  const auto calib = load<float>(dir, "calib");

  sdso_shim::Device dev(0);
  FrameHessian fh, fh_right;
  fh.slot = 100; fh_right.slot = 101;
  std::vector<int> ws(levels), hs(levels);
  std::vector<std::vector<float>> lv(levels);
  std::vector<const float*> p(levels);
  for (int l = 0; l < levels; l++) { ws[l] = w >> l; hs[l] = h >> l; lv[l] = load<float>(dir, "left_dI" + std::to_string(l)); p[l] = lv[l].data(); }
  dev.check(sdso_upload_pyramid(dev.ctx(), fh.slot, levels, ws.data(), hs.data(), p.data()), "sdso_upload_pyramid");
  const auto R = load<float>(dir, "right");
  const float* pr = R.data();
  dev.check(sdso_upload_pyramid(dev.ctx(), fh_right.slot, 1, &w, &h, &pr), "sdso_upload_pyramid");

  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  std::vector<FrameHessian*> frameHessians;
  sdso_shim::PixelSelector pixelSelector(dev);
  sdso_shim::ImmaturePoints<FrameHessian, CalibHessian, Mat33f> imm(dev, pixelSelector, Hcalib, frameHessians, [](const FrameHessian* f) { return f->slot; }, calib[4],
                                                                    calib[5]);
  Mat idepthMap(h, w);
  imm.makeNewTraces(&fh, &fh_right, nullptr);
  const int counter = imm.stereoMatch(&fh, &fh_right, idepthMap);
  if (!fh.immaturePoints.empty()) { std::fprintf(stderr, "stereoMatch built ImmaturePoint objects\n"); return 1; }
  const int before = imm.count(&fh);
  imm.release(&fh);
  std::vector<float> packed((size_t)w * h * 3);
  for (int y = 0; y < h; y++) std::memcpy(&packed[(size_t)y * w * 3], idepthMap.data + y * idepthMap.step, sizeof(float) * 3 * w);
  for (int y = 0; y < h; y++)
    for (size_t k = sizeof(float) * 3 * w; k < idepthMap.step; k++)
      if (idepthMap.data[y * idepthMap.step + k]) { std::fprintf(stderr, "stereoMatch wrote into the padding of a row\n"); return 1; }
  dump(dir, "map", packed);
  dump(dir, "counter", &counter, 1);
  std::printf("matches %d points %d %d\n", counter, before, imm.count(&fh));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_stereo_match_shim run <dir>\n");
  return 2;
}
