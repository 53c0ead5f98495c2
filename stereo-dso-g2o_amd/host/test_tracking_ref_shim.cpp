// sdso_shim::CoarseTracker::setCoarseTrackingRef on the device-resident window against the overload that walks the pointer graph, on
// stand-ins for the reference's types.  tests/test_tracking_ref_shim_gpu.py writes a window as raw arrays and runs this program twice:
//   test_tracking_ref_shim <dir> window   WindowedBA::writeBackProjections = false, optimize, setCoarseTrackingRef(ba, frameHessians, fh_right)
//   test_tracking_ref_shim <dir> graph    the full write-back, optimize, setCoarseTrackingRef(frameHessians, fh_right, Hcalib)
// and compares the template levels each run leaves (out_<mode>_*.bin) bit for bit.  FrameHessian::pointHessians of one host is NOT in
// the window's point order (two entries swapped, meta[8..9]): the splat order is pointHessians order in both runs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include "sdso_shim.h"

template <class T>
static std::vector<T> load(const std::string& dir, const char* name) {
  std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "missing %s\n", name); std::exit(2); }
  const size_t bytes = (size_t)f.tellg();
  std::vector<T> v(bytes / sizeof(T));
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), bytes);
  return v;
}
template <class T>
static void dump(const std::string& dir, const std::string& name, const std::vector<T>& v) {
  std::ofstream f(dir + "/out_" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

// ---- stand-ins with the reference's member names (HessianBlocks.h, Residuals.h, EnergyFunctionalStructs.h, EnergyFunctional.h)
struct Mat33 { double m[9]; double& operator()(int i, int j) { return m[i * 3 + j]; } double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct SE3 {
  Mat33 R; Vec3 t;
  SE3() { for (int i = 0; i < 9; i++) R.m[i] = (i % 4 == 0); t = {{0, 0, 0}}; }
  SE3(const Mat33& R_, const Vec3& t_) : R(R_), t(t_) {}
  const Mat33& rotationMatrix() const { return R; }
  const Vec3& translation() const { return t; }
};
struct AffLight { double a = 0, b = 0; };
struct Vec3f { float v[3]; };
struct Vec10 { double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct VecC { double v[4] = {0, 0, 0, 0}; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct Vec2f { float v[2] = {0, 0}; float& operator[](int i) { return v[i]; } };
struct Vec3fv { float v[3] = {0, 0, 0}; float& operator[](int i) { return v[i]; } };
struct CalibHessian {
  VecC value_scaled, value_zero, value, step;
  void setValue(const VecC& val) { value = val; for (int i = 0; i < 4; i++) value_scaled[i] = 50.0 * val[i]; }   // HessianBlocks.h:318-333 (SCALE_F = SCALE_C = 50)
  float fxl() const { return (float)value_scaled[0]; }           // value_scaledf (HessianBlocks.h:296-299)
  float fyl() const { return (float)value_scaled[1]; }
  float cxl() const { return (float)value_scaled[2]; }
  float cyl() const { return (float)value_scaled[3]; }
};
struct FrameShell { int id = 0; };
struct PointHessian;
struct FrameHessian {
  Vec3f* dIp[SDSO_PYR_LEVELS];
  std::vector<float> store[SDSO_PYR_LEVELS];
  SE3 worldToCam_evalPT; Vec10 state, state_zero, step;
  float ab_exposure = 1, frameEnergyTH = 0; int frameID = 0, slot = 0;
  FrameShell shell_store; FrameShell* shell = &shell_store;
  std::vector<PointHessian*> pointHessians;
  const SE3& get_worldToCam_evalPT() const { return worldToCam_evalPT; }
  const Vec10& get_state() const { return state; }
  const Vec10& get_state_zero() const { return state_zero; }
  void setState(const Vec10& s) { state = s; }
  void setEvalPT(const SE3& T, const Vec10& s) { worldToCam_evalPT = T; state = s; state_zero = s; }
  AffLight aff_g2l() const { return AffLight{10.0 * state[6], 1000.0 * state[7]}; }   // get_state_scaled()[6], [7] (SCALE_A, SCALE_B)
};
struct EFFrame; struct EFPoint; struct EFResidual;
struct PointFrameResidual {
  int state_state = 0, state_NewState = 0;
  double state_energy = 0, state_NewEnergy = 0, state_NewEnergyWithOutlier = 0;
  bool isNew = true;
  Vec2f projectedTo[SDSO_MAX_RES];
  Vec3fv centerProjectedTo;
  PointHessian* point = nullptr; EFResidual* efResidual = nullptr;
};
struct PointHessian {
  float u, v, idepth, idepth_zero, color[8], weights[8], step = 0, idepth_hessian = 0, maxRelBaseline = 0;
  int numGoodResiduals = 0;
  bool hasDepthPrior = false;
  std::vector<PointFrameResidual*> residuals;
  std::pair<PointFrameResidual*, int> lastResiduals[2] = {{nullptr, 2}, {nullptr, 2}};
  EFPoint* efPoint = nullptr;
  void setIdepth(float x) { idepth = x; }
  void setIdepthZero(float x) { idepth_zero = x; }
};
struct EFResidual { PointFrameResidual* data; EFFrame* target; bool isActiveAndIsGoodNEW = false; int idxInAll = 0; EFPoint* point = nullptr; bool isLinearized = false; };
struct EFPoint { PointHessian* data; std::vector<EFResidual*> residualsAll; float HdiF = 0, bdSumF = 0, deltaF = 0; EFFrame* host = nullptr; };
struct EFFrame { FrameHessian* data; std::vector<EFPoint*> points; int idx; };
struct DynMat {
  int n = 0; std::vector<double> d;
  void resize(int r, int c) { n = c; d.assign((size_t)r * c, 0.0); }
  double& operator()(int i, int j) { return d[(size_t)i * n + j]; }
};
struct EnergyFunctional {
  std::vector<EFFrame*> frames; DynMat HM, lastHS; std::vector<double> bM, lastbS, lastX;
  int resInA = 0, resInL = 0, resInM = 0;
  void dropResidual(EFResidual* r) {                             // semantics of EnergyFunctional.cpp:524-551
    auto& l = r->point->residualsAll;
    l[r->idxInAll] = l.back(); l[r->idxInAll]->idxInAll = r->idxInAll; l.pop_back();
    r->data->efResidual = nullptr;
    delete r;
  }
};
using Tracker = sdso_shim::CoarseTracker<SE3, AffLight, Mat33, Vec3>;

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: test_tracking_ref_shim <dir> window|graph\n"); return 2; }
  const std::string dir = argv[1], mode = argv[2];
  const bool from_window = mode == "window";
  if (!from_window && mode != "graph") { std::fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
  try {
    sdso_shim::Device dev(0);
    auto meta = load<int>(dir, "meta");                          // nf np nr w h its solverMode levels swapA swapB
    const int nf = meta[0], np = meta[1], nr = meta[2], w = meta[3], h = meta[4], levels = meta[7];
    auto calib = load<double>(dir, "calib");                     // value_scaled(4) value_zero(4) baseline
    auto evalPT = load<double>(dir, "evalPT"), state = load<double>(dir, "state"), state_zero = load<double>(dir, "state_zero");
    auto exposure = load<float>(dir, "ab_exposure"), eTH = load<float>(dir, "frameEnergyTH");
    auto frameID = load<int>(dir, "frameID"), res_point = load<int>(dir, "res_point"), res_target = load<int>(dir, "res_target"), host = load<int>(dir, "host");
    auto u = load<float>(dir, "u"), v = load<float>(dir, "v"), idepth = load<float>(dir, "idepth"), idz = load<float>(dir, "idepth_zero"),
         color = load<float>(dir, "color"), weights = load<float>(dir, "weights");
    auto prior = load<uint8_t>(dir, "hasDepthPrior"), res_state = load<uint8_t>(dir, "res_state");
    std::vector<std::unique_ptr<FrameHessian>> fhs;
    std::vector<std::unique_ptr<EFFrame>> effs;
    std::vector<std::unique_ptr<PointHessian>> phs;
    EnergyFunctional ef;
    CalibHessian HC;
    std::vector<int> wv(levels), hv(levels);
    for (int l = 0; l < levels; l++) { wv[l] = w >> l; hv[l] = h >> l; }
    for (int f = 0; f <= nf; f++) {                              // frame nf on file: the right image of the newest keyframe
      fhs.emplace_back(new FrameHessian);
      FrameHessian& fh = *fhs.back();
      for (int l = 0; l < levels; l++) {
        char nm[32]; std::snprintf(nm, sizeof nm, "img%d_l%d", f, l);
        fh.store[l] = load<float>(dir, nm);
        fh.dIp[l] = reinterpret_cast<Vec3f*>(fh.store[l].data());
      }
      fh.slot = 10 + f;
      dev.uploadFrame(fh.slot, &fh, levels, wv.data(), hv.data());
      if (f == nf) break;
      for (int i = 0; i < 9; i++) fh.worldToCam_evalPT.R.m[i] = evalPT[f * 12 + i];
      for (int i = 0; i < 3; i++) fh.worldToCam_evalPT.t.v[i] = evalPT[f * 12 + 9 + i];
      for (int i = 0; i < 10; i++) { fh.state[i] = state[f * 10 + i]; fh.state_zero[i] = state_zero[f * 10 + i]; }
      fh.ab_exposure = exposure[f]; fh.frameEnergyTH = eTH[f]; fh.frameID = frameID[f]; fh.shell->id = 100 + f;
      effs.emplace_back(new EFFrame{&fh, {}, f});
      ef.frames.push_back(effs.back().get());
    }
    std::vector<PointFrameResidual*> by_id(nr, nullptr);         // the residual objects the optimize call leaves alive, by window index
    int r = 0;
    for (int p = 0; p < np; p++) {
      phs.emplace_back(new PointHessian);
      PointHessian& ph = *phs.back();
      ph.u = u[p]; ph.v = v[p]; ph.idepth = idepth[p]; ph.idepth_zero = idz[p]; ph.hasDepthPrior = prior[p] != 0;
      for (int k = 0; k < 8; k++) { ph.color[k] = color[p * 8 + k]; ph.weights[k] = weights[p * 8 + k]; }
      EFPoint* efp = new EFPoint{&ph, {}};
      efp->host = effs[host[p]].get();
      ph.efPoint = efp;
      for (; r < nr && res_point[r] == p; r++) {
        PointFrameResidual* pfr = new PointFrameResidual;
        pfr->state_state = (int)res_state[r]; pfr->point = &ph;
        EFResidual* efr = new EFResidual{pfr, effs[res_target[r]].get()};
        efr->point = efp; efr->idxInAll = (int)efp->residualsAll.size();
        pfr->efResidual = efr;
        efp->residualsAll.push_back(efr);
        ph.residuals.push_back(pfr);
        if (res_target[r] == nf - 1) ph.lastResiduals[0] = {pfr, (int)res_state[r]};   // FullSystem.cpp:1370-1387: the residual into the new keyframe
      }
      efp->host->points.push_back(efp);
      fhs[host[p]]->pointHessians.push_back(&ph);
    }
    {  // pointHessians order != EFFrame::points order for one host (what flagPointsForRemoval + removePoint leave behind)
      const int a = meta[8], b = meta[9];
      if (host[a] != host[b]) throw sdso_shim::Error("the two swapped points must share their host");
      auto& l = fhs[host[a]]->pointHessians;
      std::swap(*std::find(l.begin(), l.end(), phs[a].get()), *std::find(l.begin(), l.end(), phs[b].get()));
    }
    const int n = 8 * nf + 4;
    ef.HM.resize(n, n); ef.bM.assign(n, 0.0);
    for (int i = 0; i < 4; i++) { HC.value_scaled[i] = calib[i]; HC.value_zero[i] = calib[4 + i]; }
    auto slot_of_fh = [](FrameHessian* fh) { return fh->slot; };

    sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, 0);
    ba.writeBackProjections = !from_window;
    ba.upload(&ef, &HC, w, h, /*solverMode=*/meta[6], 1e12, 1e8, true, slot_of_fh);
    ba.optimize(meta[5], &ef, &HC);
    int cpt_written = 0;                                         // residual objects whose centerProjectedTo the optimize call filled
    for (auto& ph : phs) for (PointFrameResidual* pfr : ph->residuals) cpt_written += pfr->centerProjectedTo[2] != 0.f;

    std::vector<FrameHessian*> frameHessians;
    for (int f = 0; f < nf; f++) frameHessians.push_back(fhs[f].get());
    FrameHessian* fh_right = fhs[nf].get();
    Tracker trk(dev, /*ref_slot=*/1);
    trk.slot_of = [](const void* fh) { return static_cast<const FrameHessian*>(fh)->slot; };
    trk.baseline = (float)calib[8];
    if (from_window) trk.setCoarseTrackingRef(ba, frameHessians, fh_right);
    else trk.setCoarseTrackingRef(frameHessians, fh_right, HC);

    std::vector<int> pcn(trk.pc_n, trk.pc_n + levels);
    for (int l = 0; l < levels; l++) {
      int nn = -1;
      dev.check(sdso_track_get_ref(dev.ctx(), 1, l, &nn, nullptr, nullptr, nullptr, nullptr), "sdso_track_get_ref");
      if (nn != pcn[l]) throw sdso_shim::Error("pc_n of the tracker differs from the installed template's");
      std::vector<float> lv((size_t)4 * nn);
      if (nn) dev.check(sdso_track_get_ref(dev.ctx(), 1, l, &nn, lv.data(), lv.data() + nn, lv.data() + 2 * (size_t)nn, lv.data() + 3 * (size_t)nn), "sdso_track_get_ref");
      dump(dir, mode + "_l" + std::to_string(l), lv);
    }
    dump(dir, mode + "_pcn", pcn);
    std::vector<double> info = {(double)trk.refFrameID, trk.firstCoarseRMSE, trk.lastRef_aff_g2l.a, trk.lastRef_aff_g2l.b, (double)trk.params().ref_exposure,
                                trk.params().ref_aff_g2l.a, trk.params().ref_aff_g2l.b, (double)trk.n_points, (double)trk.n_border, (double)cpt_written,
                                (double)ba.lastRemoved};
    dump(dir, mode + "_info", info);
    std::printf("%s: pc_n[0] %d, centerProjectedTo written back for %d residuals\n", mode.c_str(), pcn[0], cpt_written);
    for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) { for (EFResidual* er : p->residualsAll) { delete er->data; delete er; } delete p; }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_tracking_ref_shim: %s\n", e.what());
    return 1;
  }
  return 0;
}
