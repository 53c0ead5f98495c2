// Driver for the device-to-device keyframe hand-over of sdso_shim.h on stand-in types: CoarseDistanceMap::makeDistanceMap(WindowedBA&, ...)
// reads the seeds of the map from the resident window, ImmaturePoints::activatePointsMT runs on that map, and
// WindowedBA::updateActivated takes the activated points into the window from the activation's records.  The caller's loop over the
// records touches their integer members only: the PointHessians it inserts carry no float of the activation, and the window must still
// hold them.  tests/test_activated_shim_gpu.py writes the inputs, runs this program and compares what it dumps with the C-ABI route.
//   test_activated_shim run <dir>
// The window: the files of WindowGraph (driver_io.h).  The activation walks the window's frames (its frame k is window frame k); its own
// inputs carry the prefix a_: a_meta = minObs; a_calib = fx fy cx cy minActDist minTraceQuality; a_poses = nf x {worldToCam 12, camToWorld
// 12} doubles; a_flagged; a_pair_R / a_pair_t / a_pair_aff; a_frame<k> = the level-0 image the activation reads for frame k (pyramid slot
// 300 + k: the two halves of the test need no geometric relation, so they do not share images); a_group<k>_f / a_group<k>_st.
#include <cstdio>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

static int run(const std::string& dir) {
  sdso_shim::Device dev(0);
  WindowGraph G;
  G.build(dir, WindowGraph::Options());
  const int nf = G.nf, w = G.w, h = G.h;
  EnergyFunctional& ef = G.ef;
  int wv[1] = {w}, hv[1] = {h};
  for (FrameHessian* fh : G.fhs) dev.uploadFrame(fh->slot, fh, 1, wv, hv);
  auto slot_of = [](FrameHessian* fh) { return fh->slot; };
  sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, 0);
  ba.upload(&ef, &G.HC, w, h, /*solverMode=*/G.meta[6], 1e12, 1e8, true, slot_of);

  // ---- the activation's view of the same frames
  const int minObs = load<int>(dir, "a_meta")[0];
  const auto calib = load<float>(dir, "a_calib");
  const auto poses = load<double>(dir, "a_poses");
  const auto flagged = load<uint8_t>(dir, "a_flagged");
  const auto pR = load<float>(dir, "a_pair_R"), pt = load<float>(dir, "a_pair_t"), pa = load<float>(dir, "a_pair_aff");
  std::vector<FrameHessian*> frameHessians(G.fhs.begin(), G.fhs.begin() + nf);
  for (int k = 0; k < nf; k++) {
    FrameHessian& fh = *frameHessians[k];
    fh.PRE_worldToCam = se3_of(&poses[24 * k]); fh.PRE_camToWorld = se3_of(&poses[24 * k + 12]);
    fh.flaggedForMarginalization = flagged[k] != 0;
    fh.targetPrecalc.resize(nf);
    for (int t = 0; t < nf; t++) {
      FrameFramePrecalc& pre = fh.targetPrecalc[t];
      const size_t q = (size_t)k * nf + t;
      for (int i = 0; i < 9; i++) pre.PRE_RTll.m[i] = pR[q * 9 + i];
      for (int i = 0; i < 3; i++) pre.PRE_tTll[i] = pt[q * 3 + i];
      pre.PRE_aff_mode[0] = pa[q * 2]; pre.PRE_aff_mode[1] = pa[q * 2 + 1];
    }
    const auto img = load<float>(dir, "a_frame" + std::to_string(k));
    const float* p = img.data();
    dev.check(sdso_upload_pyramid(dev.ctx(), 300 + k, 1, &w, &h, &p), "sdso_upload_pyramid");
    if (k == nf - 1) break;
    const auto gf = load<float>(dir, "a_group" + std::to_string(k) + "_f");
    const auto gs = load<uint8_t>(dir, "a_group" + std::to_string(k) + "_st");
    for (size_t i = 0; i < gs.size(); i++) {
      ImmaturePoint* ip = new ImmaturePoint();
      point_from_record(ip, &gf[i * 30], gs[i]);
      ip->host = &fh; ip->idxInImmaturePoints = (int)i;
      fh.immaturePoints.push_back(ip);
    }
  }
  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  sdso_shim::PixelSelector pixelSelector(dev);
  using Imm = sdso_shim::ImmaturePoints<FrameHessian, CalibHessian, Mat33f>;
  Imm imm(dev, pixelSelector, Hcalib, frameHessians, [](const FrameHessian* f) { return 300 + f->idx; }, 0.f, 0.f);
  for (int k = 0; k + 1 < nf; k++) {
    imm.upload(frameHessians[k], w, h);
    for (ImmaturePoint* p : frameHessians[k]->immaturePoints) delete p;
    frameHessians[k]->immaturePoints.clear();
  }

  // ---- makeKeyFrame's two call sites: the map from the window, then the activation into the window
  sdso_shim::CoarseDistanceMap<Mat33f> cdm(dev, w, h);
  cdm.makeK(&Hcalib, 2, w, h);
  FrameHessian* newestHs = frameHessians.back();
  cdm.makeDistanceMap(ba, frameHessians, newestHs);
  std::vector<float> geoms;
  for (int k = 0; k + 1 < nf; k++) {
    const sdso_distmap_geom_t g = cdm.geomOf(frameHessians[k], newestHs);
    geoms.insert(geoms.end(), g.KRKi, g.KRKi + 9); geoms.insert(geoms.end(), g.Kt, g.Kt + 3);
  }
  dump(dir, "geoms", geoms);
  std::vector<int> items = {cdm.numItems};
  dump(dir, "num_items", items);
  dump(dir, "map0", cdm.distFinal(), (size_t)(w / 2) * (h / 2));

  const std::vector<Imm::Activated> optimized = imm.activatePointsMT(cdm, frameHessians, calib[4], calib[5], minObs);
  // the caller's loop (FullSystemOptPoint.cpp:196-237, FullSystem.cpp:919-945) on the integer members alone
  int next_res = G.nr, made = 0;
  std::vector<int> rec_i;
  for (const Imm::Activated& a : optimized) {
    rec_i.push_back(a.host->idx); rec_i.push_back(a.status);
    if (a.status != 1) continue;
    PointHessian* ph = G.addPoint(a.host->idx);                     // u, v, idepth, colour, weights stay zero: the device has them
    for (int f = 0; f < nf; f++)
      if (a.res_state[f] == ResState::IN) G.addResidual(ph, f, next_res++);
    made++;
  }
  dump(dir, "rec_i", rec_i);
  const std::vector<int> act_index = ba.updateActivated(&ef, slot_of, frameHessians, optimized.size());
  dump(dir, "act_index", act_index);

  // ---- what the window holds and computes now
  std::vector<int> o_points, o_res;
  for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) { o_points.push_back(p->data->id); for (EFResidual* er : p->residualsAll) o_res.push_back(er->data->id); }
  std::vector<int> g_frames(nf), g_points(ef.nPoints), g_res(ef.nResiduals);
  dev.check(sdso_ba_window_get_order(dev.ctx(), 0, g_frames.data(), g_points.data(), g_res.data()), "sdso_ba_window_get_order");
  std::vector<double> o_state(nf * 10);
  std::vector<float> o_idepth(ef.nPoints);
  std::vector<uint8_t> o_rstate(ef.nResiduals);
  dev.check(sdso_ba_get_state(dev.ctx(), 0, o_state.data(), o_idepth.data(), o_rstate.data()), "sdso_ba_get_state");
  std::vector<double> o_energy = {ba.linearizeAll()};
  ba.applyRes(); ba.accumulateAll();
  MatXX H3[3]; VecX b3[3];
  ba.accumulateAF_MT(H3[0], b3[0], false); ba.accumulateLF_MT(H3[1], b3[1], false); ba.accumulateSCF_MT(H3[2], b3[2], false);
  std::vector<double> o_st;
  for (int k = 0; k < 3; k++) { o_st.insert(o_st.end(), H3[k].d.begin(), H3[k].d.end()); o_st.insert(o_st.end(), b3[k].d.begin(), b3[k].d.end()); }
  dump(dir, "ef_points", o_points); dump(dir, "ef_res", o_res); dump(dir, "order_points", g_points); dump(dir, "order_res", g_res);
  dump(dir, "idepth", o_idepth); dump(dir, "rstate", o_rstate); dump(dir, "energy", o_energy); dump(dir, "stitched", o_st);
  dump(dir, "map", cdm.distFinal(), (size_t)(w / 2) * (h / 2));
  std::printf("activated %zu records, %d points, nPoints %d nResiduals %d\n", optimized.size(), made, ef.nPoints, ef.nResiduals);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "test_activated_shim: %s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_activated_shim run <dir>\n");
  return 2;
}
