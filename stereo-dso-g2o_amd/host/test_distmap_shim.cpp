// Driver for sdso_shim::CoarseDistanceMap, selectPointsToActivate and updateMinActDist on stand-in types that carry the reference's
// member names (Eigen / Sophus are not available here).  tests/test_distmap_shim_gpu.py writes the inputs as raw arrays, runs this
// program and compares what it dumps with the C-ABI path; `minact` needs no device.
//   test_distmap_shim minact <current> <desired> n1 n2 ...      one line per n: currentMinActDist after STEP 1
//   test_distmap_shim run <dir>                                 makeK, makeDistanceMap, addIntoDistFinal, STEP 2
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sdso_shim.h"
#include "driver_io.h"

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");   // w h levels nf
  const int w = meta[0], h = meta[1], levels = meta[2], nf = meta[3];
  const auto calib = load<float>(dir, "calib");
  const auto w2c = load<double>(dir, "worldToCam"), c2w = load<double>(dir, "camToWorld");
  const auto flagged = load<uint8_t>(dir, "flagged");
  const auto a_host = load<int>(dir, "a_host");
  const auto a_u = load<float>(dir, "a_u"), a_v = load<float>(dir, "a_v"), a_id = load<float>(dir, "a_idepth");
  const auto c_host = load<int>(dir, "c_host"), c_st = load<int>(dir, "c_status");
  const auto c_u = load<float>(dir, "c_u"), c_v = load<float>(dir, "c_v"), c_min = load<float>(dir, "c_idepth_min"), c_max = load<float>(dir, "c_idepth_max"),
             c_q = load<float>(dir, "c_quality"), c_itv = load<float>(dir, "c_interval"), c_ty = load<float>(dir, "c_my_type");
  const auto par = load<float>(dir, "par");   // currentMinActDist, setting_minTraceQuality
  const auto add = load<int>(dir, "add");     // pairs (u, v)

  std::vector<FrameHessian> frames(nf);
  std::vector<FrameHessian*> frameHessians;
  for (int f = 0; f < nf; f++) {
    frames[f].PRE_worldToCam = se3_of(&w2c[12 * f]);
    frames[f].PRE_camToWorld = se3_of(&c2w[12 * f]);
    frames[f].flaggedForMarginalization = f < nf - 1 && flagged[f] != 0;
    frameHessians.push_back(&frames[f]);
  }
  std::vector<PointHessian> phs(a_u.size());
  for (size_t i = 0; i < a_u.size(); i++) { phs[i].u = a_u[i]; phs[i].v = a_v[i]; phs[i].idepth_scaled = a_id[i]; frames[a_host[i]].pointHessians.push_back(&phs[i]); }
  const int nc = (int)c_u.size();
  std::vector<ImmaturePoint*> all(nc);
  for (int i = 0; i < nc; i++) {
    ImmaturePoint* p = all[i] = new ImmaturePoint();
    p->u = c_u[i]; p->v = c_v[i]; p->idepth_min = c_min[i]; p->idepth_max = c_max[i]; p->quality = c_q[i]; p->lastTracePixelInterval = c_itv[i];
    p->my_type = c_ty[i]; p->lastTraceStatus = c_st[i]; p->host = &frames[c_host[i]]; p->idxInImmaturePoints = -1; p->id = i;
    frames[c_host[i]].immaturePoints.push_back(all[i]);
  }

  sdso_shim::Device dev(0);
  sdso_shim::CoarseDistanceMap<Mat33f> cdm(dev, w, h);
  CalibHessian Hcalib(calib[0], calib[1], calib[2], calib[3]);
  cdm.makeK(&Hcalib, levels, w, h);
  const size_t npix = (size_t)cdm.w[1] * cdm.h[1];
  std::vector<sdso_distmap_geom_t> geoms;
  for (int f = 0; f < nf - 1; f++) geoms.push_back(cdm.geomOf(&frames[f], &frames[nf - 1]));
  dump(dir, "geoms", reinterpret_cast<const float*>(geoms.data()), geoms.size() * 12);

  cdm.makeDistanceMap(frameHessians, &frames[nf - 1]);
  dump(dir, "map0", cdm.distFinal(), npix);
  const int numItems = cdm.numItems;
  for (size_t i = 0; i + 1 < add.size(); i += 2) cdm.addIntoDistFinal(add[i], add[i + 1]);
  dump(dir, "map1", cdm.distFinal(), npix);

  cdm.makeDistanceMap(frameHessians, &frames[nf - 1]);
  // the deleted candidates are gone after the call: remember who sits where first
  std::vector<std::vector<int>> ids(nf);
  for (int f = 0; f < nf; f++) for (auto* p : frames[f].immaturePoints) ids[f].push_back(p->id);
  std::vector<ImmaturePoint*> toOptimize = sdso_shim::selectPointsToActivate(cdm, frameHessians, par[0], par[1]);
  std::vector<uint8_t> decision(nc, 0);
  std::vector<int> order;
  for (int f = 0; f < nf; f++)
    for (size_t i = 0; i < frames[f].immaturePoints.size(); i++) {
      ImmaturePoint* p = frames[f].immaturePoints[i];
      if (p == 0) decision[ids[f][i]] = 1;
      else if (f < nf - 1 && p->idxInImmaturePoints != (int)i) { std::fprintf(stderr, "idxInImmaturePoints not set\n"); return 1; }
    }
  for (auto* p : toOptimize) { decision[p->id] = 2; order.push_back(p->id); }
  dump(dir, "decision", decision.data(), decision.size());
  dump(dir, "order", order.data(), order.size());
  dump(dir, "map2", cdm.distFinal(), npix);
  std::printf("numItems %d toOptimize %d\n", numItems, (int)toOptimize.size());
  for (int f = 0; f < nf; f++) for (auto* p : frames[f].immaturePoints) delete p;
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "minact")) {
    for (int i = 4; i < argc; i++) {
      float c = (float)std::atof(argv[2]);
      sdso_shim::updateMinActDist(c, std::atoi(argv[i]), (float)std::atof(argv[3]));
      std::printf("%.9g\n", c);
    }
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_distmap_shim minact <current> <desired> n... | run <dir>\n");
  return 2;
}
