// Driver for sdso_shim::CoarseInitializer on stand-in types that carry the reference's member names (Eigen / Sophus are not available here).
// tests/test_init_shim_gpu.py writes the inputs as raw arrays, runs this program and compares what it dumps.
//   test_init_shim run <dir>
// meta = w h levels; calib = fx fy cx cy baseline setting_desiredPointDensity; left_dI<l> = the pyramid of the first frame; right = level 0
// of the first right frame.  Two routes in one process, each with the process's real rand():
//   shim    : setFirstStereo, points0, initializeFromInitializer(setting_desiredPointDensity / numPoints[0])
//   restated: the loops of CoarseInitializer.cpp:848-972 and FullSystem.cpp:1533-1573 written out over sdso_pixel_select,
//             sdso_immature_init_batch and sdso_trace_stereo_batch, the second ImmaturePoint and its trace included
// Dumped per route: the Pnts (u v idepth iR my_type outlierTH isGood), the points (24 words each), the draw that follows the route; the
// shim's members; the draw after setFirstStereo next to the one after srand(3141592) and w*h draws.
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

using Init = sdso_shim::CoarseInitializer<FrameHessian, CalibHessian, SE3>;

static void seed_like_pixel_selector(int w, int h) {   // PixelSelector::PixelSelector, PixelSelector2.cpp:43-45
  std::srand(3141592);
  for (int i = 0; i < w * h; i++) std::rand();
}
static void push_point(std::vector<float>& out, int pnt, float u, float v, float ty, float idepth, float imin, float imax, float eth, const float* col, const float* wgt) {
  float id;
  std::memcpy(&id, &pnt, sizeof(float));
  const float head[8] = {id, u, v, ty, idepth, imin, imax, eth};
  out.insert(out.end(), head, head + 8);
  out.insert(out.end(), col, col + 8);
  out.insert(out.end(), wgt, wgt + 8);
}
// ImmaturePoint(x, y, frame, type) with the interval 0 / NaN for every pixel, then traceStereo(right, K, 1)
struct Traced { std::vector<float> col, wgt, gH, eth, imin, imax, ids; std::vector<uint8_t> st; };
static Traced trace_fresh(sdso_shim::Device& dev, int slot_l, int slot_r, const float K4[4], float baseline, std::vector<float>& u, std::vector<float>& v) {
  const int n = (int)u.size();
  Traced T{std::vector<float>((size_t)n * 8), std::vector<float>((size_t)n * 8), std::vector<float>((size_t)n * 4), std::vector<float>(n), std::vector<float>(n, 0.f),
           std::vector<float>(n, NAN), std::vector<float>(n, 0.f), std::vector<uint8_t>(n)};
  dev.check(sdso_immature_init_batch(dev.ctx(), slot_l, n, u.data(), v.data(), T.col.data(), T.wgt.data(), T.gH.data(), T.eth.data()), "sdso_immature_init_batch");
  std::vector<float> imin0(n, 0.f), q(n, 10000.f), uv((size_t)n * 2, 0.f), itv(n, 0.f);
  std::vector<uint8_t> lts(n, 5);
  sdso_trace_points_t P{n, u.data(), v.data(), imin0.data(), T.imin.data(), T.imax.data(), T.ids.data(), T.col.data(), T.wgt.data(), T.gH.data(), T.eth.data(),
                        q.data(), lts.data(), uv.data(), itv.data()};
  dev.check(sdso_trace_stereo_batch(dev.ctx(), slot_r, K4, baseline, 1, &P, T.st.data()), "sdso_trace_stereo_batch");
  return T;
}

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");
  const int w = meta[0], h = meta[1], levels = meta[2];
  const auto calib = load<float>(dir, "calib");
  const float baseline = calib[4], desired = calib[5];

  sdso_shim::Device dev(0);
  FrameHessian left, right;
  left.slot = 100; right.slot = 101;
  {
    std::vector<std::vector<float>> lv(levels);
    std::vector<const float*> p(levels);
    std::vector<int> ws(levels), hs(levels);
    for (int l = 0; l < levels; l++) { ws[l] = w >> l; hs[l] = h >> l; lv[l] = load<float>(dir, "left_dI" + std::to_string(l)); p[l] = lv[l].data(); }
    dev.check(sdso_upload_pyramid(dev.ctx(), left.slot, levels, ws.data(), hs.data(), p.data()), "sdso_upload_pyramid");
    const auto R = load<float>(dir, "right");
    const float* pr = R.data();
    dev.check(sdso_upload_pyramid(dev.ctx(), right.slot, 1, &w, &h, &pr), "sdso_upload_pyramid");
  }
  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  const float K4[4] = {Hcalib.fxl(), Hcalib.fyl(), Hcalib.cxl(), Hcalib.cyl()};

  // ---- the shim.  Members that setFirstStereo must reset are set to something else first, and the generator is somewhere else.
  Init ci(dev, w, h, [](const FrameHessian* f) { return f->slot; }, baseline);
  ci.thisToNext.t[0] = 3; ci.snapped = true; ci.frameID = 7; ci.snappedAt = 5;
  std::srand(12345);
  ci.setFirstStereo(&Hcalib, &left, &right);
  const int draw_shim = std::rand();
  seed_like_pixel_selector(w, h);
  const int draw_ref = std::rand();
  std::srand(999);
  ci.setFirstStereo(&Hcalib, &left, &right);       // once more, so that STEP 3 draws from where setFirstStereo leaves the generator
  const std::vector<Init::Pnt> pnts = ci.points0();
  const float keepPercentage = desired / ci.numPoints[0];                            // FullSystem.cpp:1525
  const std::vector<Init::Point> pts = ci.initializeFromInitializer(keepPercentage);
  const int after_shim = std::rand();
  {
    std::vector<float> f;
    for (const auto& p : pnts) { const float r[7] = {p.u, p.v, p.idepth, p.iR, p.my_type, p.outlierTH, p.isGood ? 1.f : 0.f}; f.insert(f.end(), r, r + 7); }
    dump(dir, "shim_pnts", f);
    f.clear();
    for (const auto& p : pts) push_point(f, p.pnt, p.u, p.v, p.my_type, p.idepth, p.idepth_min, p.idepth_max, p.energyTH, p.color, p.weights);
    dump(dir, "shim_points", f);
    const int members[6] = {ci.numPoints[0], ci.frameID, ci.snapped ? 1 : 0, ci.snappedAt, ci.firstFrame == &left ? 1 : 0, ci.firstRightFrame == &right ? 1 : 0};
    dump(dir, "members", members, 6);
    std::vector<double> T(ci.thisToNext.R.m, ci.thisToNext.R.m + 9);
    for (int i = 0; i < 3; i++) T.push_back(ci.thisToNext.t[i]);
    dump(dir, "thisToNext", T);
  }

  // ---- restated: setFirstStereo, level 0 (CoarseInitializer.cpp:848-972)
  seed_like_pixel_selector(w, h);                                                    // `PixelSelector sel(w[0], h[0])`
  std::vector<float> statusMap((size_t)w * h);
  int potential = 3, npts = 0;                                                       // sel.currentPotential = 3
  dev.check(sdso_pixel_select(dev.ctx(), left.slot, 0.03f * w * h, 1, 2.f, &potential, statusMap.data(), &npts), "sdso_pixel_select");
  std::vector<float> us, vs, types;
  for (int y = 3; y < h - 4; y++)
    for (int x = 3; x < w - 4; x++)
      if (statusMap[x + (size_t)y * w] != 0) { us.push_back((float)x); vs.push_back((float)y); types.push_back(statusMap[x + (size_t)y * w]); }
  const int nl = (int)us.size();
  const Traced T1 = trace_fresh(dev, left.slot, right.slot, K4, baseline, us, vs);
  std::vector<float> f, iR(nl);
  for (int i = 0; i < nl; i++) {
    iR[i] = T1.st[i] == 0 ? T1.ids[i] : 0.01f;
    const float r[7] = {us[i], vs[i], iR[i], iR[i], types[i], 8 * (12.f * 12.f), 1.f};
    f.insert(f.end(), r, r + 7);
  }
  dump(dir, "ref_pnts", f);
  // ---- restated: initializeFromInitializer STEP 3 (FullSystem.cpp:1533-1573).  The only rand() of the loop stands at its top, so the
  // draws are made first, in order, and the points that pass take their constructor and their trace in one batch.
  const float keepRef = desired / nl;
  std::vector<int> walked;
  std::vector<float> u2, v2;
  for (int i = 0; i < nl; i++) {
    if (std::rand() / (float)RAND_MAX > keepRef) continue;
    walked.push_back(i);
    u2.push_back((float)(int)(us[i] + 0.5f)); v2.push_back((float)(int)(vs[i] + 0.5f));   // the (int u_, int v_, ...) constructor
  }
  const int after_ref = std::rand();
  const Traced T2 = trace_fresh(dev, left.slot, right.slot, K4, baseline, u2, v2);
  f.clear();
  for (size_t k = 0; k < walked.size(); k++) {
    const float idepth_min = T2.imin[k], idepth_max = T2.imax[k];
    if (!std::isfinite(T2.eth[k]) || !std::isfinite(idepth_min) || !std::isfinite(idepth_max) || idepth_min < 0 || idepth_max < 0) continue;
    push_point(f, walked[k], u2[k], v2[k], types[walked[k]], T2.ids[k], idepth_min, idepth_max, T2.eth[k], &T2.col[k * 8], &T2.wgt[k * 8]);
  }
  dump(dir, "ref_points", f);
  const int draws[6] = {draw_shim, draw_ref, after_shim, after_ref, npts, nl};
  dump(dir, "draws", draws, 6);
  std::printf("pnts %d %d points %zu %zu\n", (int)pnts.size(), nl, pts.size(), f.size() / 24);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_init_shim run <dir>\n");
  return 2;
}
