// Driver for sdso_shim::ImmaturePoints on stand-in types that carry the reference's member names (Eigen / Sophus are not available here).
// tests/test_immature_shim_gpu.py writes the inputs as raw arrays, runs this program and compares what it dumps with the C-ABI path.
//   test_immature_shim run <dir>
// meta = w h levels nhosts nframes; calib = fx fy cx cy baseline density; poses = (nhosts + nframes) x {worldToCam 12, camToWorld 12} doubles;
// affs = (nhosts + nframes) x {a, b, exposure} doubles; host<k>_dI<l> = the pyramid of host k; frame<k>_left / _right = level 0 of frame k;
// flags = the removal mask of host 0 after the traces.  A first frame without makeNewTraces heads frameHessians; makeNewTraces for every host, traceNewCoarseNonKey for every frame but the last,
// traceNewCoarseKey for the last, download, remove, download.  Dumped: K, Ki, the geometries of every frame, every member of every point.
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");
  const int w = meta[0], h = meta[1], levels = meta[2], nh = meta[3], nfr = meta[4];
  const auto calib = load<float>(dir, "calib");
  const auto poses = load<double>(dir, "poses");
  const auto affs = load<double>(dir, "affs");
  const auto flags = load<uint8_t>(dir, "flags");

  sdso_shim::Device dev(0);
  std::vector<FrameHessian> hosts(nh), lefts(nfr), rights(nfr);
  auto setup = [&](FrameHessian& fh, int k, int slot) {
    fh.PRE_worldToCam = se3_of(&poses[24 * k]); fh.PRE_camToWorld = se3_of(&poses[24 * k + 12]);
    fh.aff = AffLight{affs[3 * k], affs[3 * k + 1]}; fh.ab_exposure = (float)affs[3 * k + 2];
    fh.slot = slot;
  };
  std::vector<int> ws(levels), hs(levels);
  for (int l = 0; l < levels; l++) { ws[l] = w >> l; hs[l] = h >> l; }
  std::vector<FrameHessian*> frameHessians;
  for (int k = 0; k < nh; k++) {
    setup(hosts[k], k, 100 + k);
    std::vector<std::vector<float>> lv(levels);
    std::vector<const float*> p(levels);
    for (int l = 0; l < levels; l++) { lv[l] = load<float>(dir, "host" + std::to_string(k) + "_dI" + std::to_string(l)); p[l] = lv[l].data(); }
    dev.check(sdso_upload_pyramid(dev.ctx(), hosts[k].slot, levels, ws.data(), hs.data(), p.data()), "sdso_upload_pyramid");
  }
  for (int k = 0; k < nfr; k++) {
    setup(lefts[k], nh + k, 200 + 2 * k);
    setup(rights[k], nh + k, 201 + 2 * k);
    const auto L = load<float>(dir, "frame" + std::to_string(k) + "_left"), R = load<float>(dir, "frame" + std::to_string(k) + "_right");
    const float* pl = L.data();
    const float* pr = R.data();
    dev.check(sdso_upload_pyramid(dev.ctx(), lefts[k].slot, 1, &w, &h, &pl), "sdso_upload_pyramid");
    dev.check(sdso_upload_pyramid(dev.ctx(), rights[k].slot, 1, &w, &h, &pr), "sdso_upload_pyramid");
  }

  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  sdso_shim::PixelSelector pixelSelector(dev);
  sdso_shim::ImmaturePoints<FrameHessian, CalibHessian, Mat33f> imm(dev, pixelSelector, Hcalib, frameHessians, [](const FrameHessian* f) { return f->slot; }, calib[4],
                                                                    calib[5]);
  // the first keyframe: initializeFromInitializer pushes firstFrame into frameHessians without makeNewTraces (FullSystem.cpp:1487-1500) and
  // makeKeyFrame traces over it — an empty loop in the reference, no error here.  It stays in the window for every later trace.
  FrameHessian first;
  setup(first, 0, 99);
  frameHessians.push_back(&first);
  imm.traceNewCoarseKey(&lefts[0], &rights[0]);
  imm.traceNewCoarseNonKey(&lefts[0], &rights[0]);
  std::vector<int> made;
  for (int k = 0; k < nh; k++) { frameHessians.push_back(&hosts[k]); made.push_back(imm.makeNewTraces(&hosts[k], nullptr, nullptr)); }
  dump(dir, "made", made.data(), made.size());
  std::vector<float> geoms;
  for (int k = 0; k < nfr; k++)
    for (int j = 0; j < nh; j++) {
      const sdso_imm_geom_t g = imm.geomOf(&hosts[j], &lefts[k]);
      if (g.host_id != hosts[j].slot) { std::fprintf(stderr, "host_id is not the host's slot\n"); return 1; }
      geoms.insert(geoms.end(), g.KRKi, g.KRKi + 9); geoms.insert(geoms.end(), g.Kt, g.Kt + 3); geoms.insert(geoms.end(), g.aff, g.aff + 2);
      geoms.insert(geoms.end(), g.KRi, g.KRi + 9); geoms.insert(geoms.end(), g.t, g.t + 3);
    }
  dump(dir, "geoms", geoms.data(), geoms.size());
  Mat33f K, Ki;
  imm.makeK(K, Ki);
  const float kk[13] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2), Ki.m[0], Ki.m[1], Ki.m[2], Ki.m[3], Ki.m[4], Ki.m[5], Ki.m[6], Ki.m[7], Ki.m[8]};
  dump(dir, "K4Ki", kk, 13);
  for (int k = 0; k < nfr; k++) {
    if (k + 1 < nfr) imm.traceNewCoarseNonKey(&lefts[k], &rights[k]);
    else imm.traceNewCoarseKey(&lefts[k], &rights[k]);
  }
  for (int k = 0; k < nh; k++) { imm.download(&hosts[k]); dump_points(dir, "h" + std::to_string(k), hosts[k], true); }
  if ((int)flags.size() != imm.count(&hosts[0])) { std::fprintf(stderr, "flags do not fit host 0\n"); return 1; }
  imm.remove(&hosts[0], flags);
  imm.download(&hosts[0]);
  dump_points(dir, "removed", hosts[0], true);
  imm.release(&hosts[1]);
  for (int k = 0; k < nfr; k++) imm.traceNewCoarseKey(&lefts[k], &rights[k]);   // a released host is in frameHessians until the caller erases it
  imm.download(&first);
  if (!first.immaturePoints.empty()) { std::fprintf(stderr, "the first frame has points\n"); return 1; }
  std::printf("points");
  for (int k = 0; k < nh; k++) std::printf(" %d", imm.count(&hosts[k]));
  std::printf("\n");
  for (auto& fh : hosts) for (auto* p : fh.immaturePoints) delete p;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_immature_shim run <dir>\n");
  return 2;
}
