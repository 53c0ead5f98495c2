// The published map through sdso_shim::PointMap / KeyFrameDisplay on stand-ins for the reference's types, next to KeyFrameDisplay::setFromKF /
// refreshPC written out here over the same stand-ins.  tests/test_map_shim_gpu.py writes the window as raw arrays, runs this program and
// compares what the two routes leave (out_<route>_*.bin):
//   ref    upload, optimize (every member written back), the reference's removeOutliers and flagPointsForRemoval, then the literal host loops
//          of setFromKF (IOWrapper/Pangolin/KeyFrameDisplay.cpp:85-165) and refreshPC (:174-323) reading the PointHessians and ImmaturePoints
//   shim   upload, optimize, ba.removeOutliers / ba.flagPointsForRemoval, PointMap::update, KeyFrameDisplay::setFromKF / refreshPC
// Each route has its own graph and its own device window; frame 1 carries a small immature group.  The lists are dumped as records, then per
// frame four refreshPC calls: new settings, the same again, other settings with canRefresh = false, other settings — with the return values
// and the buffers after the first and the last; then the many-frames form against the ref route's loop.
// The ref route's refreshPC follows the library's stated deviations: z = depth (the rand() jitter of :246 at its mean) and no :240.
//
//   test_map_shim <dir>        files: those of WindowGraph with extras, frame_marg (nf bytes), th (scaledTH absTH minBS, floats)
#include <algorithm>
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

static float g_minIdepthH_marg = 50;
static const int patternNum = 8;
static const int patternP[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};   // settings.cpp:216

// ---- PointHessian::isOOB, removeOutliers, flagPointsForRemoval as in test_flag_points_shim.cpp, on FrameHessian's own lists
static bool isOOB(const PointHessian* ph, const std::vector<FrameHessian*>& toMarg) {                     // HessianBlocks.h:439-462
  int visInToMarg = 0;
  for (PointFrameResidual* r : ph->residuals) {
    if (r->state_state != ResState::IN) continue;
    for (FrameHessian* k : toMarg) if (r->target == k) visInToMarg++;
  }
  if ((int)ph->residuals.size() >= 3 && ph->numGoodResiduals > 4 + 10 && (int)ph->residuals.size() - visInToMarg < 3) return true;
  if (ph->lastResiduals[0].second == ResState::OOB) return true;
  if (ph->residuals.size() < 2) return false;
  if (ph->lastResiduals[0].second == ResState::OUTLIER && ph->lastResiduals[1].second == ResState::OUTLIER) return true;
  return false;
}
static void removeOutliers_ref(std::vector<FrameHessian*>& frameHessians) {                               // FullSystemOptimize.cpp:1063-1084
  for (FrameHessian* fh : frameHessians)
    for (unsigned int i = 0; i < fh->pointHessians.size(); i++) {
      PointHessian* ph = fh->pointHessians[i];
      if (ph == 0) continue;
      if (ph->residuals.size() == 0) {
        fh->pointHessiansOut.push_back(ph);
        ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
        fh->pointHessians[i] = fh->pointHessians.back();
        fh->pointHessians.pop_back();
        i--;
      }
    }
}
static void flagPointsForRemoval_ref(std::vector<FrameHessian*>& frameHessians) {                         // FullSystem.cpp:965-1056
  std::vector<FrameHessian*> fhsToMargPoints;
  for (FrameHessian* fh : frameHessians) if (fh->flaggedForMarginalization) fhsToMargPoints.push_back(fh);
  for (FrameHessian* host : frameHessians) {
    for (unsigned int i = 0; i < host->pointHessians.size(); i++) {
      PointHessian* ph = host->pointHessians[i];
      if (ph == 0) continue;
      if (ph->idepth_scaled < 0 || ph->residuals.size() == 0) {
        host->pointHessiansOut.push_back(ph);
        ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
        host->pointHessians[i] = 0;
      } else if (isOOB(ph, fhsToMargPoints) || host->flaggedForMarginalization) {
        if (ph->isInlierNew() && ph->idepth_hessian > g_minIdepthH_marg) {
          ph->efPoint->stateFlag = EFPointStatus::PS_MARGINALIZE;
          host->pointHessiansMarginalized.push_back(ph);
        } else {
          ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
          host->pointHessiansOut.push_back(ph);
        }
        host->pointHessians[i] = 0;
      }
    }
    for (int i = 0; i < (int)host->pointHessians.size(); i++)
      if (host->pointHessians[i] == 0) {
        host->pointHessians[i] = host->pointHessians.back();
        host->pointHessians.pop_back();
        i--;
      }
  }
}

// ---- KeyFrameDisplay (IOWrapper/Pangolin/KeyFrameDisplay.h / .cpp), the members and the two functions this test is about
struct InputPointSparse { float u, v, idpeth, idepth_hessian, relObsBaseline; int numGoodRes; unsigned char status; };   // KeyFrameDisplay.h:37-48; its float color[ppp] is color_f below
struct RefDisplay {
  int id = 0;
  float fx, fy, cx, cy, fxi, fyi, cxi, cyi;
  SE3 camToWorld;
  bool needRefresh = true;
  float my_scaledTH = 1e10, my_absTH = 1e10, my_minRelBS = 0;
  int my_displayMode = 1, my_sparsifyFactor = 1;
  std::vector<InputPointSparse> originalInputSparse;
  int numSparsePoints = 0, numGLBufferGoodPoints = 0;
  bool bufferValid = false;
  std::vector<float> vertexBuffer;             // the two GL buffers
  std::vector<unsigned char> colorBuffer;
  std::vector<float> color_f;                  // InputPointSparse<ppp>::color, 8 floats per point

  void setFromKF(FrameHessian* fh, CalibHessian* HCalib) {
    id = fh->shell->id;                                                                                    // setFromF, :68-83
    fx = HCalib->fxl(); fy = HCalib->fyl(); cx = HCalib->cxl(); cy = HCalib->cyl();
    fxi = 1 / fx; fyi = 1 / fy; cxi = -cx / fx; cyi = -cy / fy;
    originalInputSparse.clear(); color_f.clear();
    auto push = [&](const float* color, float u, float v, float idepth, float bs, float idh, int good, int status) {
      InputPointSparse pc{};
      for (int i = 0; i < patternNum; i++) color_f.push_back(color[i]);
      pc.u = u; pc.v = v; pc.idpeth = idepth; pc.relObsBaseline = bs; pc.idepth_hessian = idh; pc.numGoodRes = good; pc.status = (unsigned char)status;
      originalInputSparse.push_back(pc);
    };
    for (ImmaturePoint* p : fh->immaturePoints) push(p->color, p->u, p->v, (p->idepth_max + p->idepth_min) * 0.5f, 0, 1000, 1, 0);   // :104-117
    for (PointHessian* p : fh->pointHessians) push(p->color, p->u, p->v, p->idepth_scaled, p->maxRelBaseline, p->idepth_hessian, 0, 1);             // :119-132
    for (PointHessian* p : fh->pointHessiansMarginalized) push(p->color, p->u, p->v, p->idepth_scaled, p->maxRelBaseline, p->idepth_hessian, 0, 2); // :134-146
    for (PointHessian* p : fh->pointHessiansOut) push(p->color, p->u, p->v, p->idepth_scaled, p->maxRelBaseline, p->idepth_hessian, 0, 3);          // :148-160
    numSparsePoints = (int)originalInputSparse.size();
    camToWorld = fh->PRE_camToWorld;
    needRefresh = true;
  }
  bool refreshPC(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    if (canRefresh)
      needRefresh = needRefresh || my_scaledTH != scaledTH || my_absTH != absTH || my_displayMode != mode || my_minRelBS != minBS || my_sparsifyFactor != sparsity;
    if (!needRefresh) return false;
    needRefresh = false;
    my_scaledTH = scaledTH; my_absTH = absTH; my_displayMode = mode; my_minRelBS = minBS; my_sparsifyFactor = sparsity;
    if (numSparsePoints == 0) return false;
    std::vector<float> tmpVertexBuffer((size_t)numSparsePoints * patternNum * 3);
    std::vector<unsigned char> tmpColorBuffer((size_t)numSparsePoints * patternNum * 3);
    int vertexBufferNumPoints = 0;
    for (int i = 0; i < numSparsePoints; i++) {
      if (my_displayMode == 1 && originalInputSparse[i].status != 1 && originalInputSparse[i].status != 2) continue;
      if (my_displayMode == 2 && originalInputSparse[i].status != 1) continue;
      if (my_displayMode > 2) continue;
      if (originalInputSparse[i].idpeth < 0) continue;
      float depth = 1.0f / originalInputSparse[i].idpeth;
      float depth4 = depth * depth;
      depth4 *= depth4;
      float var = (1.0f / (originalInputSparse[i].idepth_hessian + 0.01));
      if (var * depth4 > my_scaledTH) continue;
      if (var > my_absTH) continue;
      if (originalInputSparse[i].relObsBaseline < my_minRelBS) continue;
      for (int pnt = 0; pnt < patternNum; pnt++) {
        int dx = patternP[pnt][0];
        int dy = patternP[pnt][1];
        float* V = &tmpVertexBuffer[(size_t)vertexBufferNumPoints * 3];
        unsigned char* C = &tmpColorBuffer[(size_t)vertexBufferNumPoints * 3];
        V[0] = ((originalInputSparse[i].u + dx) * fxi + cxi) * depth;
        V[1] = ((originalInputSparse[i].v + dy) * fyi + cyi) * depth;
        V[2] = depth;                                                                                      // (:246 without the jitter)
        if (my_displayMode == 0) {
          const int st = originalInputSparse[i].status;
          C[0] = st == 3 ? 255 : 0; C[1] = (st == 0 || st == 1) ? 255 : 0; C[2] = (st == 0 || st == 2) ? 255 : 0;   // :252-275
        } else {
          C[0] = C[1] = C[2] = (unsigned char)color_f[(size_t)i * patternNum + pnt];
        }
        vertexBufferNumPoints++;
      }
    }
    if (vertexBufferNumPoints == 0) return true;
    numGLBufferGoodPoints = vertexBufferNumPoints;
    vertexBuffer.assign(tmpVertexBuffer.begin(), tmpVertexBuffer.begin() + (size_t)vertexBufferNumPoints * 3);
    colorBuffer.assign(tmpColorBuffer.begin(), tmpColorBuffer.begin() + (size_t)vertexBufferNumPoints * 3);
    bufferValid = true;
    return true;
  }
};

using BA = sdso_shim::WindowedBA<EnergyFunctional, CalibHessian>;
using ShimDisplay = sdso_shim::KeyFrameDisplay<FrameHessian, CalibHessian>;
static const int IMM_FRAME = 1, IMM_N = 37;

// a small immature group on frame IMM_FRAME: every third point not traced yet (idepth_max NaN, ImmaturePoint.cpp:34)
static void make_immature(FrameHessian* fh) {
  for (int i = 0; i < IMM_N; i++) {
    ImmaturePoint* p = new ImmaturePoint();
    p->u = 20.f + 11.f * i; p->v = 30.f + 7.f * i; p->u_stereo = p->u; p->v_stereo = p->v; p->host = fh; p->idxInImmaturePoints = i; p->id = i;
    p->idepth_min = i % 3 == 0 ? 0.f : 0.1f + 0.01f * i; p->idepth_max = i % 3 == 0 ? NAN : 0.5f + 0.02f * i;
    p->idepth_min_stereo = p->idepth_min; p->idepth_max_stereo = p->idepth_max; p->idepth_stereo = 0;
    for (int k = 0; k < 8; k++) { p->color[k] = 3.5f * i + 17.25f * k; p->weights[k] = 1.f; }
    p->gradH(0, 0) = p->gradH(1, 1) = 1.f; p->energyTH = 100.f; p->quality = 3.f; p->my_type = 1.f;
    p->lastTraceStatus = 0; p->lastTracePixelInterval = 0;
    fh->immaturePoints.push_back(p);
  }
}
static void put_immature(sdso_shim::Device& dev, const FrameHessian* fh, int w, int h) {
  const int n = (int)fh->immaturePoints.size();
  std::vector<float> u(n), v(n), ty(n), imin(n), imax(n), q(n), col(n * 8), wgt(n * 8), gH(n * 4), eth(n), uv(n * 2), itv(n);
  std::vector<uint8_t> st(n);
  for (int i = 0; i < n; i++) {
    const ImmaturePoint* p = fh->immaturePoints[i];
    u[i] = p->u; v[i] = p->v; ty[i] = p->my_type; imin[i] = p->idepth_min; imax[i] = p->idepth_max; q[i] = p->quality; eth[i] = p->energyTH;
    for (int k = 0; k < 8; k++) { col[i * 8 + k] = p->color[k]; wgt[i * 8 + k] = p->weights[k]; }
    gH[i * 4] = gH[i * 4 + 3] = 1.f;
  }
  sdso_trace_points_t P{n, u.data(), v.data(), nullptr, imin.data(), imax.data(), nullptr, col.data(), wgt.data(), gH.data(), eth.data(), q.data(), st.data(), uv.data(), itv.data()};
  dev.check(sdso_imm_put_host(dev.ctx(), fh->slot, w, h, &P, ty.data()), "sdso_imm_put_host");
}

static void push_record(std::vector<float>& o, const PointHessian* p) {                                   // the record of sdso_abi.h from the members :121-129 read
  o.push_back(p->u); o.push_back(p->v); o.push_back(p->idepth_scaled); o.push_back(p->idepth_hessian); o.push_back(p->maxRelBaseline);
  for (int k = 0; k < 8; k++) o.push_back(p->color[k]);
  for (int k = 0; k < 3; k++) o.push_back(0.f);
}

static void run_route(sdso_shim::Device& dev, const std::string& dir, const std::string& tag, int win_id, bool use_shim) {
  WindowGraph G;
  WindowGraph::Options opt;
  opt.extras = true; opt.last_state_from_file = true; opt.point_hessians = true;
  G.build(dir, opt);
  EnergyFunctional& ef = G.ef;
  const auto frame_marg = load<uint8_t>(dir, "frame_marg");
  const auto th = load<float>(dir, "th");
  std::vector<FrameHessian*> frameHessians(G.fhs.begin(), G.fhs.begin() + G.nf);
  for (int f = 0; f < G.nf; f++) {
    G.fhs[f]->flaggedForMarginalization = frame_marg[f] != 0;
    std::reverse(G.fhs[f]->pointHessians.begin(), G.fhs[f]->pointHessians.end());                          // list order != window order
    for (int i = 0; i < 3; i++) { G.fhs[f]->PRE_camToWorld.t[i] = 0.5 * f + i; }
  }
  make_immature(G.fhs[IMM_FRAME]);
  int wv[1] = {G.w}, hv[1] = {G.h};
  for (FrameHessian* fh : G.fhs) dev.uploadFrame(fh->slot, fh, 1, wv, hv);
  auto slot_of = [](FrameHessian* fh) { return fh->slot; };

  BA ba(dev, win_id);
  ba.writeBackProjections = false;
  ba.upload(&ef, &G.HC, G.w, G.h, /*solverMode=*/G.meta[6], 1e12, 1e8, true, slot_of);
  ba.optimize(G.meta[5], &ef, &G.HC);
  if (tag == "ref") {                                          // the threshold of both routes, as in test_flag_points_shim.cpp
    std::vector<float> h;
    for (PointHessian* ph : G.phs) if (ph->idepth_hessian > 0) h.push_back(ph->idepth_hessian);
    if (h.empty()) throw std::runtime_error("no positive idepth_hessian");
    std::nth_element(h.begin(), h.begin() + (h.size() - 1) / 2, h.end());
    g_minIdepthH_marg = h[(h.size() - 1) / 2];
  }
  ba.setting_minIdepthH_marg = g_minIdepthH_marg;

  sdso_shim::PointMap map(dev);
  if (use_shim) {
    put_immature(dev, G.fhs[IMM_FRAME], G.w, G.h);
    ba.removeOutliers(frameHessians);
    ba.flagPointsForRemoval(frameHessians);
    map.update(ba, frameHessians);
  } else {
    removeOutliers_ref(frameHessians);
    flagPointsForRemoval_ref(frameHessians);
  }
  // ---- the lists as records
  std::vector<int> counts;
  for (int l = 1; l <= 3; l++) {
    std::vector<float> rec;
    for (FrameHessian* fh : frameHessians) {
      const auto& list = l == 1 ? fh->pointHessians : l == 2 ? fh->pointHessiansMarginalized : fh->pointHessiansOut;
      if (use_shim) { const auto r = map.records(fh->frameID, l); rec.insert(rec.end(), r.begin(), r.end()); counts.push_back((int)r.size() / 16); }
      else { for (const PointHessian* p : list) push_record(rec, p); counts.push_back((int)list.size()); }
    }
    dump(dir, tag + "_list" + std::to_string(l), rec);
  }
  dump(dir, tag + "_counts", counts);
  // ---- per frame: four refreshPC calls
  const float scaledTH = th[0], absTH = th[1], minBS = th[2];
  auto imm_of = [](const FrameHessian* fh) { return fh->immaturePoints.empty() ? -1 : fh->slot; };
  std::vector<int> rets, good;
  std::vector<float> v1, v4, vm;
  std::vector<unsigned char> c1, c4, cm;
  std::vector<ShimDisplay*> shim_displays;
  std::vector<RefDisplay> ref_displays(G.nf);
  for (int f = 0; f < G.nf; f++) {
    FrameHessian* fh = frameHessians[f];
    auto run4 = [&](auto& D, const std::vector<float>& V, const auto& C) {
      rets.push_back(D.refreshPC(true, scaledTH, absTH, 1, minBS, 1));                                     // new settings
      good.push_back(D.numGLBufferGoodPoints);
      v1.insert(v1.end(), V.begin(), V.end()); c1.insert(c1.end(), C.begin(), C.end());
      rets.push_back(D.refreshPC(true, scaledTH, absTH, 1, minBS, 1));                                     // unchanged
      rets.push_back(D.refreshPC(false, scaledTH * 2, 1.0f, 0, 0.f, 1));                                  // changed, but canRefresh = false
      rets.push_back(D.refreshPC(true, scaledTH * 2, 1.0f, 0, 0.f, 1));                                    // changed: absTH = 1 lets the immature points (var = 1 / 1000.01) through
      good.push_back(D.numGLBufferGoodPoints);
      v4.insert(v4.end(), V.begin(), V.end()); c4.insert(c4.end(), C.begin(), C.end());
      rets.push_back(D.id);
    };
    if (use_shim) {
      ShimDisplay* D = new ShimDisplay(dev, imm_of);
      shim_displays.push_back(D);
      D->setFromKF(fh, &G.HC);
      run4(*D, D->vertices(), D->colors());
      if (D->camToWorld.t[0] != fh->PRE_camToWorld.t[0]) throw std::runtime_error("camToWorld is not PRE_camToWorld");
    } else {
      RefDisplay& D = ref_displays[f];
      D.setFromKF(fh, &G.HC);
      run4(D, D.vertexBuffer, D.colorBuffer);
    }
  }
  // ---- a whole publishKeyframes call: setFromKF on every frame, then mode 2
  if (use_shim) {
    for (int f = 0; f < G.nf; f++) shim_displays[f]->setFromKF(frameHessians[f], &G.HC);
    const std::vector<bool> r = ShimDisplay::refreshPC(shim_displays, true, scaledTH, absTH, 2, minBS, 1);
    for (int f = 0; f < G.nf; f++) {
      rets.push_back(r[f]); good.push_back(shim_displays[f]->numGLBufferGoodPoints);
      vm.insert(vm.end(), shim_displays[f]->vertices().begin(), shim_displays[f]->vertices().end());
      cm.insert(cm.end(), shim_displays[f]->colors().begin(), shim_displays[f]->colors().end());
    }
    bool threw = false;
    try { shim_displays[0]->refreshPC(true, scaledTH, absTH, 1, minBS, 2); } catch (const sdso_shim::Error&) { threw = true; }
    if (!threw) throw std::runtime_error("refreshPC with sparsity = 2 did not throw");
    std::printf("sparsity 2 refused\n");
    // a refresh the device refuses leaves needRefresh set on every display it did not rebuild: the last frame leaves the map, a call over
    // frames 0 and nf-1 with new settings throws, and frame 0 — whose turn had come first — still rebuilds for those settings afterwards
    map.release(frameHessians[G.nf - 1]->frameID);
    std::vector<ShimDisplay*> two{shim_displays[0], shim_displays[G.nf - 1]};
    for (int rep = 0; rep < 2; rep++) {
      threw = false;
      try { ShimDisplay::refreshPC(two, true, scaledTH * 3, absTH, 1, minBS, 1); } catch (const sdso_shim::Error&) { threw = true; }
      if (!threw) throw std::runtime_error("refreshPC over a released keyframe did not throw");
    }
    if (!shim_displays[0]->refreshPC(true, scaledTH * 3, absTH, 1, minBS, 1)) throw std::runtime_error("a refused refresh cleared needRefresh");
    if (shim_displays[0]->refreshPC(true, scaledTH * 3, absTH, 1, minBS, 1)) throw std::runtime_error("an unchanged refresh rebuilt");
    std::printf("refused refresh kept needRefresh\n");
    for (ShimDisplay* D : shim_displays) delete D;
  } else {
    for (int f = 0; f < G.nf; f++) {
      RefDisplay& D = ref_displays[f];
      D.setFromKF(frameHessians[f], &G.HC);
      rets.push_back(D.refreshPC(true, scaledTH, absTH, 2, minBS, 1)); good.push_back(D.numGLBufferGoodPoints);
      vm.insert(vm.end(), D.vertexBuffer.begin(), D.vertexBuffer.end()); cm.insert(cm.end(), D.colorBuffer.begin(), D.colorBuffer.end());
    }
  }
  dump(dir, tag + "_rets", rets); dump(dir, tag + "_good", good);
  dump(dir, tag + "_v1", v1); dump(dir, tag + "_c1", c1); dump(dir, tag + "_v4", v4); dump(dir, tag + "_c4", c4); dump(dir, tag + "_vm", vm); dump(dir, tag + "_cm", cm);
  int tot[3] = {0, 0, 0};
  for (int l = 0; l < 3; l++) for (int f = 0; f < G.nf; f++) tot[l] += counts[l * G.nf + f];
  std::printf("%s: points active %d marginalised %d out %d, vertices %zu / %zu / %zu\n", tag.c_str(), tot[0], tot[1], tot[2], v1.size() / 3, v4.size() / 3, vm.size() / 3);
  for (ImmaturePoint* p : G.fhs[IMM_FRAME]->immaturePoints) delete p;
  G.fhs[IMM_FRAME]->immaturePoints.clear();
  if (use_shim) {
    dev.check(sdso_imm_release_host(dev.ctx(), G.fhs[IMM_FRAME]->slot), "sdso_imm_release_host");
    for (FrameHessian* fh : frameHessians) map.release(fh->frameID);                                   // (releasing the last one again is not an error)
  }
  dev.check(sdso_ba_release_window(dev.ctx(), win_id), "sdso_ba_release_window");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_map_shim <dir>\n"); return 2; }
  const std::string dir = argv[1];
  try {
    sdso_shim::Device dev(0);
    run_route(dev, dir, "ref", 0, false);
    run_route(dev, dir, "shim", 1, true);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_map_shim: %s\n", e.what());
    return 1;
  }
  return 0;
}
