// FullSystem::removeOutliers / flagPointsForRemoval through sdso_shim::WindowedBA on stand-ins for the reference's types, next to the
// reference's two functions written out here over the same stand-ins.  tests/test_flag_points_shim_gpu.py writes the window as raw arrays,
// runs this program and compares what the routes leave (out_<route>_*.bin):
//   ref    upload, optimize (every member written back), the reference's removeOutliers and flagPointsForRemoval below, reading
//          residuals.size(), idepth_scaled, numGoodResiduals, idepth_hessian and lastResiduals of the PointHessians
//   shim   upload, optimize, ba.removeOutliers / ba.flagPointsForRemoval (the device decides)
//   nowb   the same with writeBackPointStats = false: the PointHessians keep the uploaded idepth_hessian / maxRelBaseline / numGoodResiduals
// Every route then goes on the same way: willDropPoints + dropPointsF (one sweep for the PS_DROP points of both functions), update(),
// marginalizePointsF; HM / bM are dumped.
// Each route has its own graph and its own device window.  setting_minIdepthH_marg is the lower median of the positive idepth_hessian the
// `ref` route's optimize wrote back (the synthetic Hessians are ~1e7: the default of 50 would never drop a weak point), so one point sits
// exactly on the threshold.
//
//   test_flag_points_shim <dir>        files: those of WindowGraph with extras, and frame_marg (nf bytes)
#include <algorithm>
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

// FrameHessian's lists of the two functions (HessianBlocks.h:119-123); standins.h carries pointHessians only
struct KeyFrame {
  FrameHessian* fh = nullptr;
  bool flaggedForMarginalization = false;
  std::vector<PointHessian*> pointHessians, pointHessiansMarginalized, pointHessiansOut;
};

static float g_minIdepthH_marg = 50;
static const int setting_minGoodActiveResForMarg = 3, setting_minGoodResForMarg = 4;   // settings.cpp:82-83

// PointHessian::isOOB (HessianBlocks.h:439-462)
static bool isOOB(const PointHessian* ph, const std::vector<FrameHessian*>& /*toKeep*/, const std::vector<FrameHessian*>& toMarg) {
  int visInToMarg = 0;
  for (PointFrameResidual* r : ph->residuals) {
    if (r->state_state != ResState::IN) continue;
    for (FrameHessian* k : toMarg)
      if (r->target == k) visInToMarg++;
  }
  if ((int)ph->residuals.size() >= setting_minGoodActiveResForMarg && ph->numGoodResiduals > setting_minGoodResForMarg + 10 &&
      (int)ph->residuals.size() - visInToMarg < setting_minGoodActiveResForMarg)
    return true;
  if (ph->lastResiduals[0].second == ResState::OOB) return true;
  if (ph->residuals.size() < 2) return false;
  if (ph->lastResiduals[0].second == ResState::OUTLIER && ph->lastResiduals[1].second == ResState::OUTLIER) return true;
  return false;
}

struct RefCounters { int numPointsDropped = 0, flag_oob = 0, flag_in = 0, flag_inin = 0, flag_nores = 0; };

// FullSystem::removeOutliers (FullSystemOptimize.cpp:1063-1084) up to ef->dropPointsF(), which every route's caller runs after flagPointsForRemoval
static void removeOutliers_ref(std::vector<KeyFrame*>& frameHessians, RefCounters& C) {
  for (KeyFrame* fh : frameHessians)
    for (unsigned int i = 0; i < fh->pointHessians.size(); i++) {
      PointHessian* ph = fh->pointHessians[i];
      if (ph == 0) continue;
      if (ph->residuals.size() == 0) {
        fh->pointHessiansOut.push_back(ph);
        ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
        fh->pointHessians[i] = fh->pointHessians.back();
        fh->pointHessians.pop_back();
        i--;
        C.numPointsDropped++;
      }
    }
}

// FullSystem::flagPointsForRemoval (FullSystem.cpp:965-1056) without :1012-1021 (WindowedBA::marginalizePointsF holds them)
static void flagPointsForRemoval_ref(std::vector<KeyFrame*>& frameHessians, RefCounters& C) {
  std::vector<FrameHessian*> fhsToKeepPoints, fhsToMargPoints;
  for (int i = ((int)frameHessians.size()) - 1; i >= 0 && i >= ((int)frameHessians.size()); i--)
    if (!frameHessians[i]->flaggedForMarginalization) fhsToKeepPoints.push_back(frameHessians[i]->fh);
  for (int i = 0; i < (int)frameHessians.size(); i++)
    if (frameHessians[i]->flaggedForMarginalization) fhsToMargPoints.push_back(frameHessians[i]->fh);
  for (KeyFrame* host : frameHessians) {
    for (unsigned int i = 0; i < host->pointHessians.size(); i++) {
      PointHessian* ph = host->pointHessians[i];
      if (ph == 0) continue;
      if (ph->idepth_scaled < 0 || ph->residuals.size() == 0) {
        host->pointHessiansOut.push_back(ph);
        ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
        host->pointHessians[i] = 0;
        C.flag_nores++;
      } else if (isOOB(ph, fhsToKeepPoints, fhsToMargPoints) || host->flaggedForMarginalization) {
        C.flag_oob++;
        if (ph->isInlierNew()) {
          C.flag_in++;
          if (ph->idepth_hessian > g_minIdepthH_marg) {
            C.flag_inin++;
            ph->efPoint->stateFlag = EFPointStatus::PS_MARGINALIZE;
            host->pointHessiansMarginalized.push_back(ph);
          } else {
            ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
            host->pointHessiansOut.push_back(ph);
          }
        } else {
          host->pointHessiansOut.push_back(ph);
          ph->efPoint->stateFlag = EFPointStatus::PS_DROP;
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

using BA = sdso_shim::WindowedBA<EnergyFunctional, CalibHessian>;

// the lists of every host as point ids, each list behind its length
static std::vector<int> lists_of(const std::vector<KeyFrame*>& kfs, std::vector<PointHessian*> KeyFrame::*member) {
  std::vector<int> o;
  for (const KeyFrame* kf : kfs) {
    o.push_back((int)(kf->*member).size());
    for (const PointHessian* ph : kf->*member) o.push_back(ph->id);
  }
  return o;
}

static void run_route(sdso_shim::Device& dev, const std::string& dir, const std::string& tag, int win_id, bool use_shim, bool write_back) {
  WindowGraph G;
  WindowGraph::Options opt;
  opt.extras = true; opt.last_state_from_file = true; opt.point_hessians = true;
  G.build(dir, opt);
  EnergyFunctional& ef = G.ef;
  const auto frame_marg = load<uint8_t>(dir, "frame_marg");
  std::vector<KeyFrame> store(G.nf);
  std::vector<KeyFrame*> frameHessians;
  for (int f = 0; f < G.nf; f++) {
    G.fhs[f]->flaggedForMarginalization = frame_marg[f] != 0;
    store[f].fh = G.fhs[f]; store[f].flaggedForMarginalization = frame_marg[f] != 0; store[f].pointHessians = G.fhs[f]->pointHessians;
    frameHessians.push_back(&store[f]);
  }
  int wv[1] = {G.w}, hv[1] = {G.h};
  for (FrameHessian* fh : G.fhs) dev.uploadFrame(fh->slot, fh, 1, wv, hv);
  auto slot_of = [](FrameHessian* fh) { return fh->slot; };
  auto is_drop = [](EFPoint* p) { return p->stateFlag == PS_DROP; };

  BA ba(dev, win_id);
  ba.writeBackPointStats = write_back;
  ba.writeBackProjections = false;
  ba.upload(&ef, &G.HC, G.w, G.h, /*solverMode=*/G.meta[6], 1e12, 1e8, true, slot_of);
  ba.optimize(G.meta[5], &ef, &G.HC);
  if (!write_back)                                           // the members the decisions would be read from are NOT there
    for (PointHessian* ph : G.phs) if (ph->idepth_hessian != 0) throw std::runtime_error("writeBackPointStats = false wrote idepth_hessian");
  if (tag == "ref") {                                        // the threshold of all routes
    std::vector<float> h;
    for (PointHessian* ph : G.phs) if (ph->idepth_hessian > 0) h.push_back(ph->idepth_hessian);
    if (h.empty()) throw std::runtime_error("no positive idepth_hessian");
    std::nth_element(h.begin(), h.begin() + (h.size() - 1) / 2, h.end());
    g_minIdepthH_marg = h[(h.size() - 1) / 2];
  }
  ba.setting_minIdepthH_marg = g_minIdepthH_marg;

  std::vector<int> state_flag(G.np, -1);
  auto note_flags = [&]() { for (PointHessian* ph : G.phs) if (ph->efPoint) state_flag[ph->id] = ph->efPoint->stateFlag; };
  RefCounters C;
  if (use_shim) {                                            // no decisions yet; a live lastResiduals[0] that observes frame nf-2 is refused
    bool threw = false;
    try { ba.flagPointsForRemoval(frameHessians); } catch (const sdso_shim::Error&) { threw = true; }
    if (!threw) throw std::runtime_error("flagPointsForRemoval without removeOutliers did not throw");
    PointHessian* both = nullptr;
    for (PointHessian* ph : G.phs) if (ph->lastResiduals[0].first && ph->lastResiduals[1].first) { both = ph; break; }
    if (!both) throw std::runtime_error("no point with two live lastResiduals");
    std::swap(both->lastResiduals[0], both->lastResiduals[1]);
    threw = false;
    try { ba.removeOutliers(frameHessians); } catch (const sdso_shim::Error&) { threw = true; }
    std::swap(both->lastResiduals[0], both->lastResiduals[1]);
    if (!threw) throw std::runtime_error("removeOutliers with swapped lastResiduals did not throw");
  }
  // ---- removeOutliers
  if (use_shim) { ba.removeOutliers(frameHessians); C.numPointsDropped = ba.numPointsDropped; }
  else removeOutliers_ref(frameHessians, C);
  note_flags();
  dump(dir, tag + "_ro_points", lists_of(frameHessians, &KeyFrame::pointHessians));
  dump(dir, tag + "_ro_out", lists_of(frameHessians, &KeyFrame::pointHessiansOut));
  // (removeOutliers' own ef->dropPointsF(), FullSystemOptimize.cpp:1083, waits for the one below: its points have left pointHessians, so
  // flagPointsForRemoval does not meet them, and one window edit holds one dropPointsF sweep)
  // ---- flagPointsForRemoval
  if (use_shim) { ba.flagPointsForRemoval(frameHessians); C.flag_oob = ba.flag_oob; C.flag_in = ba.flag_in; C.flag_inin = ba.flag_inin; C.flag_nores = ba.flag_nores; }
  else flagPointsForRemoval_ref(frameHessians, C);
  note_flags();
  dump(dir, tag + "_points", lists_of(frameHessians, &KeyFrame::pointHessians));
  dump(dir, tag + "_out", lists_of(frameHessians, &KeyFrame::pointHessiansOut));
  dump(dir, tag + "_marg", lists_of(frameHessians, &KeyFrame::pointHessiansMarginalized));
  dump(dir, tag + "_state_flag", state_flag);
  const std::vector<int> counters = {C.numPointsDropped, C.flag_oob, C.flag_in, C.flag_inin, C.flag_nores};
  dump(dir, tag + "_counters", counters);
  if (use_shim) {                                            // the decisions are consumed: a second call has none
    bool threw = false;
    try { ba.flagPointsForRemoval(frameHessians); } catch (const sdso_shim::Error&) { threw = true; }
    if (!threw) throw std::runtime_error("a second flagPointsForRemoval did not throw");
  }
  // ---- the keyframe goes on: dropPointsF, the window brought in line, marginalizePointsF
  ba.willDropPoints(is_drop);
  ef.dropPointsF();
  ba.update(&ef, slot_of);
  ba.marginalizePointsF(&ef, [](EFPoint* p) { return p->stateFlag == PS_MARGINALIZE; });
  dump(dir, tag + "_HM", ef.HM.d); dump(dir, tag + "_bM", ef.bM);
  std::vector<int> ef_points;
  for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) ef_points.push_back(p->data->id);
  dump(dir, tag + "_ef_points", ef_points);
  if (use_shim) {                                            // decisions of an older window do not survive update()
    bool threw = false;
    try { ba.flagPointsForRemoval(frameHessians); } catch (const sdso_shim::Error&) { threw = true; }
    if (!threw) throw std::runtime_error("flagPointsForRemoval after update() did not throw");
  }
  std::printf("%s: dropped %d flag_oob %d flag_in %d flag_inin %d flag_nores %d minIdepthH_marg %g nPoints %d resInM %d\n", tag.c_str(), C.numPointsDropped,
              C.flag_oob, C.flag_in, C.flag_inin, C.flag_nores, (double)g_minIdepthH_marg, ef.nPoints, ef.resInM);
  dev.check(sdso_ba_release_window(dev.ctx(), win_id), "sdso_ba_release_window");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_flag_points_shim <dir>\n"); return 2; }
  const std::string dir = argv[1];
  try {
    sdso_shim::Device dev(0);
    run_route(dev, dir, "ref", 0, false, true);
    run_route(dev, dir, "shim", 1, true, true);
    run_route(dev, dir, "nowb", 2, true, false);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_flag_points_shim: %s\n", e.what());
    return 1;
  }
  return 0;
}
