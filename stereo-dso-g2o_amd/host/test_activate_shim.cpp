// Driver for sdso_shim::ImmaturePoints::upload / activatePointsMT on stand-in types that carry the reference's member names (Eigen /
// Sophus are not available here).  tests/test_activate_shim_gpu.py writes the inputs as raw arrays, runs this program and compares what
// it dumps with the C-ABI path and with the CPU statement.
//   test_activate_shim run <dir>
// meta = w h nf minObs; calib = fx fy cx cy minActDist minTraceQuality; poses = nf x {worldToCam 12, camToWorld 12} doubles; flagged = nf
// bytes; pair_R / pair_t / pair_aff = the FrameFramePrecalc members, host * nf + target; frame<k> = level 0 of frame k; group<k>_f /
// group<k>_st = the immature points of frame k < nf-1 (30 floats and a status byte per point); seeds<k> = u v idepth_scaled of its
// pointHessians.  upload for every host, makeDistanceMap, activatePointsMT, the caller's loop over the records (FullSystemOptPoint.cpp:
// 196-237, FullSystem.cpp:923-933), download.  Dumped: the geometries, the records, the new pointHessians, the set afterwards, the map.
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");
  const int w = meta[0], h = meta[1], nf = meta[2], minObs = meta[3];
  const auto calib = load<float>(dir, "calib");
  const auto poses = load<double>(dir, "poses");
  const auto flagged = load<uint8_t>(dir, "flagged");
  const auto pR = load<float>(dir, "pair_R"), pt = load<float>(dir, "pair_t"), pa = load<float>(dir, "pair_aff");

  sdso_shim::Device dev(0);
  std::vector<FrameHessian> frames(nf);
  std::vector<FrameHessian*> frameHessians;
  for (int k = 0; k < nf; k++) {
    FrameHessian& fh = frames[k];
    fh.PRE_worldToCam = se3_of(&poses[24 * k]); fh.PRE_camToWorld = se3_of(&poses[24 * k + 12]);
    fh.idx = k; fh.slot = 300 + k; fh.flaggedForMarginalization = flagged[k] != 0;
    fh.targetPrecalc.resize(nf);
    for (int t = 0; t < nf; t++) {
      FrameFramePrecalc& pre = fh.targetPrecalc[t];
      const size_t q = (size_t)k * nf + t;
      for (int i = 0; i < 9; i++) pre.PRE_RTll.m[i] = pR[q * 9 + i];
      for (int i = 0; i < 3; i++) pre.PRE_tTll[i] = pt[q * 3 + i];
      pre.PRE_aff_mode[0] = pa[q * 2]; pre.PRE_aff_mode[1] = pa[q * 2 + 1];
    }
    const auto img = load<float>(dir, "frame" + std::to_string(k));
    const float* p = img.data();
    dev.check(sdso_upload_pyramid(dev.ctx(), fh.slot, 1, &w, &h, &p), "sdso_upload_pyramid");
    frameHessians.push_back(&fh);
    if (k == nf - 1) break;
    const auto gf = load<float>(dir, "group" + std::to_string(k) + "_f");
    const auto gs = load<uint8_t>(dir, "group" + std::to_string(k) + "_st");
    for (size_t i = 0; i < gs.size(); i++) {
      ImmaturePoint* ip = new ImmaturePoint();
      point_from_record(ip, &gf[i * 30], gs[i]);
      ip->host = &fh; ip->idxInImmaturePoints = (int)i;
      fh.immaturePoints.push_back(ip);
    }
    const auto sd = load<float>(dir, "seeds" + std::to_string(k));
    for (size_t i = 0; i < sd.size() / 3; i++) {
      PointHessian* ph = new PointHessian();
      ph->u = sd[3 * i]; ph->v = sd[3 * i + 1]; ph->idepth_scaled = sd[3 * i + 2]; ph->host = &fh;
      fh.pointHessians.push_back(ph);
    }
  }

  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  sdso_shim::PixelSelector pixelSelector(dev);
  using Imm = sdso_shim::ImmaturePoints<FrameHessian, CalibHessian, Mat33f>;
  Imm imm(dev, pixelSelector, Hcalib, frameHessians, [](const FrameHessian* f) { return f->slot; }, 0.f, 0.f);
  std::vector<size_t> first_new(nf, 0);
  for (int k = 0; k + 1 < nf; k++) {
    imm.upload(&frames[k], w, h);
    if (imm.count(&frames[k]) != (int)frames[k].immaturePoints.size()) { std::fprintf(stderr, "upload lost points\n"); return 1; }
    for (ImmaturePoint* p : frames[k].immaturePoints) delete p;     // from here on no ImmaturePoint object exists
    frames[k].immaturePoints.clear();
    first_new[k] = frames[k].pointHessians.size();
  }
  sdso_shim::CoarseDistanceMap<Mat33f> cdm(dev, w, h);
  cdm.makeK(&Hcalib, 2, w, h);
  FrameHessian* newestHs = frameHessians.back();
  cdm.makeDistanceMap(frameHessians, newestHs);
  std::vector<float> geoms;
  for (int k = 0; k + 1 < nf; k++) {
    const sdso_distmap_geom_t g = cdm.geomOf(&frames[k], newestHs);
    geoms.insert(geoms.end(), g.KRKi, g.KRKi + 9); geoms.insert(geoms.end(), g.Kt, g.Kt + 3);
  }
  dump(dir, "geoms", geoms.data(), geoms.size());

  const std::vector<Imm::Activated> optimized = imm.activatePointsMT(cdm, frameHessians, calib[4], calib[5], minObs);
  const size_t n = optimized.size();
  std::vector<int> ri(n * 4);
  std::vector<float> rf(n * 23);
  std::vector<uint8_t> rs(n * nf);
  // the caller's loop: the tail of optimizeImmaturePoint (FullSystemOptPoint.cpp:196-237) and STEP 4 (FullSystem.cpp:919-945)
  for (size_t k = 0; k < n; k++) {
    const Imm::Activated& a = optimized[k];
    ri[k * 4] = a.host->idx; ri[k * 4 + 1] = a.idxInImmaturePoints; ri[k * 4 + 2] = a.status; ri[k * 4 + 3] = a.lastTraceStatus;
    float* o = &rf[k * 23];
    o[0] = a.idepth; o[1] = a.u; o[2] = a.v; o[3] = a.my_type; o[4] = a.idepth_min; o[5] = a.idepth_max; o[6] = a.energyTH;
    for (int c = 0; c < 8; c++) { o[7 + c] = a.color[c]; o[15 + c] = a.weights[c]; }
    for (int f = 0; f < nf; f++) rs[k * nf + f] = a.res_state[f];
    if (a.status != 1) continue;                                    // 0 / -1: nothing to add; the entry's removal happened in the set
    PointHessian* p = new PointHessian();                           // PointHessian(point, &Hcalib), HessianBlocks.cpp:35-70
    p->host = a.host; p->u = a.u; p->v = a.v; p->my_type = a.my_type; p->energyTH = a.energyTH;
    p->idepth_scaled = (a.idepth_max + a.idepth_min) * 0.5f;
    for (int c = 0; c < 8; c++) { p->color[c] = a.color[c]; p->weights[c] = a.weights[c]; }
    p->lastResiduals[0] = {nullptr, ResState::OOB}; p->lastResiduals[1] = {nullptr, ResState::OOB};
    p->idepth_zero = p->idepth_scaled = a.idepth;                   // setIdepthZero / setIdepth (SCALE_IDEPTH = 1)
    for (int f = 0; f < nf; f++) {
      if (a.res_state[f] != ResState::IN) continue;
      PointFrameResidual* r = new PointFrameResidual;
      r->host = p->host; r->target = frameHessians[f];
      p->residuals.push_back(r);
      if (r->target == frameHessians.back()) p->lastResiduals[0] = {r, ResState::IN};
      else if (r->target == (frameHessians.size() < 2 ? nullptr : frameHessians[frameHessians.size() - 2])) p->lastResiduals[1] = {r, ResState::IN};
    }
    p->host->pointHessians.push_back(p);                            // ef->insertPoint / insertResidual follow here in the reference
  }
  dump(dir, "rec_i", ri.data(), ri.size());
  dump(dir, "rec_f", rf.data(), rf.size());
  dump(dir, "rec_rs", rs.data(), rs.size());
  for (int k = 0; k + 1 < nf; k++) {
    std::vector<float> pf;
    std::vector<int> pi;
    for (size_t i = first_new[k]; i < frames[k].pointHessians.size(); i++) {
      const PointHessian* p = frames[k].pointHessians[i];
      pf.push_back(p->u); pf.push_back(p->v); pf.push_back(p->idepth_zero);
      int mask = 0;
      for (const PointFrameResidual* r : p->residuals) mask |= 1 << r->target->idx;
      pi.push_back(mask); pi.push_back((int)p->lastResiduals[0].second); pi.push_back((int)p->lastResiduals[1].second);
    }
    dump(dir, "ph" + std::to_string(k) + "_f", pf.data(), pf.size());
    dump(dir, "ph" + std::to_string(k) + "_i", pi.data(), pi.size());
    if (!frames[k].immaturePoints.empty()) { std::fprintf(stderr, "host->immaturePoints was touched\n"); return 1; }
    imm.download(&frames[k]);
    dump_points(dir, "h" + std::to_string(k), frames[k], false);
  }
  dump(dir, "map", cdm.distFinal(), (size_t)(w / 2) * (h / 2));
  std::printf("activated %zu points", n);
  for (int k = 0; k + 1 < nf; k++) std::printf(" %d", imm.count(&frames[k]));
  std::printf("\n");
  for (auto& fh : frames) {
    for (auto* p : fh.immaturePoints) delete p;
    for (auto* p : fh.pointHessians) { for (auto* r : p->residuals) delete r; delete p; }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_activate_shim run <dir>\n");
  return 2;
}
