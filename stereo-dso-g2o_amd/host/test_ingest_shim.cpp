// Driver for sdso_shim::Undistort on stand-in types that carry the reference's member names (Eigen is not available here).
// tests/test_ingest_shim_gpu.py writes the inputs as raw arrays, runs this program and compares what it dumps with the C-ABI path.
//   test_ingest_shim run <dir>
// meta = wOrg hOrg w h bits model out_mode photometricCalibration useExposure; pars (8 doubles), out_calib (4 floats), exposure (2),
// G, vinv, raw0, raw1.  Object A is built from the model parameters, object B from A's remap tables as caller-owned arrays; A ingests the
// stereo pair in one call, B the two images one by one.  Dumped: K, size, remap tables, exposures, and every level of the four slots.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

using Undistort = sdso_shim::Undistort<Mat33, Vector2i>;

static void dump_slot(sdso_shim::Device& dev, const std::string& dir, const std::string& tag, int slot, int w, int h) {
  const int levels = sdso_pyramid_levels(w, h);
  for (int l = 0; l < levels; l++) {
    const size_t n = (size_t)(w >> l) * (h >> l);
    std::vector<float> dI(3 * n), ag(n);
    dev.check(sdso_download_pyramid_level(dev.ctx(), slot, l, dI.data()), "sdso_download_pyramid_level");
    dev.check(sdso_download_abs_grad(dev.ctx(), slot, l, ag.data()), "sdso_download_abs_grad");
    dump(dir, tag + "_dI" + std::to_string(l), dI.data(), dI.size());
    dump(dir, tag + "_ag" + std::to_string(l), ag.data(), ag.size());
  }
}

template <class T>
static int run_typed(const std::string& dir, const std::vector<int>& meta) {
  const int wOrg = meta[0], hOrg = meta[1], w = meta[2], h = meta[3], model = meta[5], out_mode = meta[6], photo = meta[7], useExposure = meta[8];
  const auto pars = load<double>(dir, "pars");
  const auto oc = load<float>(dir, "out_calib");
  const auto exposure = load<float>(dir, "exposure");
  const auto G = load<float>(dir, "G"), vinv = load<float>(dir, "vinv");
  auto raw0 = load<T>(dir, "raw0"), raw1 = load<T>(dir, "raw1");
  MinimalImage<T> left{wOrg, hOrg, raw0.data()}, right{wOrg, hOrg, raw1.data()};

  sdso_shim::Device dev(0);
  Undistort A(dev, 1, model, pars.data(), wOrg, hOrg, w, h, out_mode, oc.data(), 0.5372f);
  const Mat33 K = A.getK();
  const double k4[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
  Undistort B(dev, 2, k4, wOrg, hOrg, w, h, A.remapX(), A.remapY(), A.getBl());
  if (!A.isValid() || A.getSize()[0] != w || A.getSize()[1] != h || A.getOriginalSize()[0] != wOrg || B.getOriginalSize()[1] != hOrg || B.getBl() != 0.5372f) {
    std::fprintf(stderr, "accessors disagree with the constructor arguments\n");
    return 1;
  }
  dump(dir, "K", K.m, 9);
  dump(dir, "remapX", A.remapX(), (size_t)w * h);
  dump(dir, "remapY", A.remapY(), (size_t)w * h);
  bool threw = false;
  try { A.undistort(&left, 11, exposure[0]); } catch (const sdso_shim::Error&) { threw = true; }   // no photometric calibration loaded yet
  if (!threw) { std::fprintf(stderr, "undistort before loadPhotometricCalibration did not throw\n"); return 1; }
  A.loadPhotometricCalibration((int)sizeof(T), G.data(), vinv.data(), photo, useExposure != 0);
  B.loadPhotometricCalibration((int)sizeof(T), G.data(), vinv.data(), photo, useExposure != 0);

  float ex_out[4] = {0, 0, 0, 0};
  A.undistortStereo(&left, &right, 11, 12, exposure.data(), 1.0f, ex_out);
  ex_out[2] = B.undistort(&left, 13, exposure[0], 0.0, 1.0f);
  ex_out[3] = B.undistort(&right, 14, exposure[1], 0.0, 1.0f);
  std::fill(raw0.begin(), raw0.end(), (T)0);       // the calls only enqueued: the raw images may go away
  std::fill(raw1.begin(), raw1.end(), (T)0);
  dev.check(sdso_ctx_sync(dev.ctx()), "sdso_ctx_sync");
  dump(dir, "exposure", ex_out, 4);
  const char* tags[4] = {"a0", "a1", "b0", "b1"};
  for (int i = 0; i < 4; i++) dump_slot(dev, dir, tags[i], 11 + i, w, h);
  MinimalImage<T> small{wOrg - 1, hOrg, raw0.data()};
  threw = false;
  try { A.undistort(&small, 11, 1.0f); } catch (const sdso_shim::Error&) { threw = true; }
  if (!threw) { std::fprintf(stderr, "a wrong image size did not throw\n"); return 1; }
  std::printf("levels %d\n", sdso_pyramid_levels(w, h));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try {
      const auto meta = load<int>(argv[2], "meta");
      return meta[4] == 8 ? run_typed<unsigned char>(argv[2], meta) : run_typed<unsigned short>(argv[2], meta);
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_ingest_shim run <dir>\n");
  return 2;
}
