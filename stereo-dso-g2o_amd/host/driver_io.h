// What the test drivers share besides the stand-in types: the raw-array files the Python tests write and read (<dir>/<name>.bin in,
// <dir>/out_<name>.bin out), the 30-float immature-point record, and WindowGraph, which turns a flattened BA window into the
// reference's pointer graph.  Nothing here touches the device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include "standins.h"

template <class T>
static std::vector<T> load(const std::string& dir, const std::string& name) {
  std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "missing %s\n", name.c_str()); std::exit(2); }
  const size_t bytes = (size_t)f.tellg();
  std::vector<T> v(bytes / sizeof(T));
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}
template <class T>
static void dump(const std::string& dir, const std::string& name, const T* p, size_t n) {
  std::ofstream f(dir + "/out_" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}
template <class T>
static void dump(const std::string& dir, const std::string& name, const std::vector<T>& v) { dump(dir, name, v.data(), v.size()); }

static inline SE3 se3_of(const double* p) {   // 12 doubles: R row-major, t
  SE3 T;
  for (int i = 0; i < 9; i++) T.R.m[i] = p[i];
  for (int i = 0; i < 3; i++) T.t[i] = p[9 + i];
  return T;
}
// the pyramid of one frame from <prefix>_l<level>.bin
static inline void load_pyramid(const std::string& dir, const std::string& prefix, FrameHessian& fh, int levels) {
  fh.store.resize(levels);
  for (int l = 0; l < levels; l++) {
    fh.store[l] = load<float>(dir, prefix + "_l" + std::to_string(l));
    fh.dIp[l] = reinterpret_cast<Vec3f*>(fh.store[l].data());
  }
}

// ---- the immature-point record of tests/immature_cases.py (_pack / _unpack): 30 floats and a status byte per point
//   u v my_type idepth_min idepth_max quality color[8] weights[8] gradH(00 01 10 11) energyTH lastTraceUV[2] lastTracePixelInterval
static inline void point_from_record(ImmaturePoint* p, const float* o, uint8_t status) {
  p->u = o[0]; p->v = o[1]; p->my_type = o[2]; p->idepth_min = o[3]; p->idepth_max = o[4]; p->quality = o[5];
  for (int k = 0; k < 8; k++) { p->color[k] = o[6 + k]; p->weights[k] = o[14 + k]; }
  p->gradH(0, 0) = o[22]; p->gradH(0, 1) = o[23]; p->gradH(1, 0) = o[24]; p->gradH(1, 1) = o[25];
  p->energyTH = o[26]; p->lastTraceUV[0] = o[27]; p->lastTraceUV[1] = o[28]; p->lastTracePixelInterval = o[29];
  p->lastTraceStatus = status;
}
// out_<tag>_f / out_<tag>_st for fh.immaturePoints; check_links: every point must name fh as host and its own position
static inline void dump_points(const std::string& dir, const std::string& tag, const FrameHessian& fh, bool check_links) {
  const size_t n = fh.immaturePoints.size();
  std::vector<float> f(n * 30);
  std::vector<uint8_t> st(n);
  for (size_t i = 0; i < n; i++) {
    const ImmaturePoint* p = fh.immaturePoints[i];
    float* o = &f[i * 30];
    o[0] = p->u; o[1] = p->v; o[2] = p->my_type; o[3] = p->idepth_min; o[4] = p->idepth_max; o[5] = p->quality;
    for (int k = 0; k < 8; k++) { o[6 + k] = p->color[k]; o[14 + k] = p->weights[k]; }
    o[22] = p->gradH(0, 0); o[23] = p->gradH(0, 1); o[24] = p->gradH(1, 0); o[25] = p->gradH(1, 1);
    o[26] = p->energyTH; o[27] = p->lastTraceUV[0]; o[28] = p->lastTraceUV[1]; o[29] = p->lastTracePixelInterval;
    st[i] = (uint8_t)p->lastTraceStatus;
    if (check_links && (p->host != &fh || p->idxInImmaturePoints != (int)i)) { std::fprintf(stderr, "host / idxInImmaturePoints not set\n"); std::exit(1); }
  }
  dump(dir, tag + "_f", f);
  dump(dir, tag + "_st", st);
}

// ---- one BA window as the reference's pointer graph: FrameHessian / EFFrame / PointHessian / EFPoint / PointFrameResidual / EFResidual with
// residuals, residualsAll, idxInAll, idxInPoints, lastResiduals.  Files: meta = nf np nr w h its solverMode ...; calib = value_scaled(4)
// value_zero(4) ...; per frame evalPT(12) state(10) state_zero(10) ab_exposure frameEnergyTH frameID and img<f>_l<level>; per point host u v
// idepth idepth_zero color(8) weights(8) hasDepthPrior, grouped by host (makeIDX order); per residual res_point res_target res_state,
// grouped by point.  Frame f gets slot 10 + f, shell id 100 + f; aff_g2l() follows its state.  The graph owns every object; what
// EnergyFunctional::dropResidual / removePoint or the shim deleted has left the lists the destructor walks.
struct WindowGraph {
  struct Options {
    int levels = 1;                  // pyramid levels on file per frame
    int frames_on_file = 0;          // 0: nf.  More: frames past the window (their EFFrame is not in ef.frames); one past the per-frame
                                     // arrays has pixels only (the right image of the tracking-reference driver)
    bool extras = false;             // HM, bM, maxRelBaseline, numGoodResiduals, res_isNew are on file (else: zero prior, defaults)
    bool last_state_from_file = false;   // lastResiduals[k].second = res_state (FullSystem.cpp:1370-1387) instead of IN
    bool point_hessians = false;     // fill FrameHessian::pointHessians ...
    int swap_a = -1, swap_b = -1;    // ... with these two points of one host swapped (what flagPointsForRemoval + removePoint leave behind)
  };
  std::vector<int> meta, host;
  std::vector<double> calib;
  int nf = 0, np = 0, nr = 0, w = 0, h = 0;
  std::vector<FrameHessian*> fhs;
  std::vector<EFFrame*> effs;
  std::vector<PointHessian*> phs;             // by id; a point outlives its EFPoint
  std::vector<PointFrameResidual*> pfrs;      // by id, as built: valid until the first drop
  EnergyFunctional ef;
  CalibHessian HC;

  // PointHessian + EnergyFunctional::insertPoint (EnergyFunctional.cpp:507-521)
  PointHessian* addPoint(int host_idx) {
    PointHessian* ph = new PointHessian;
    ph->id = (int)phs.size(); ph->host = fhs[host_idx];
    EFPoint* efp = new EFPoint{ph, {}, PS_GOOD};
    efp->host = effs[host_idx]; efp->idxInPoints = (int)efp->host->points.size();
    ph->efPoint = efp;
    efp->host->points.push_back(efp);
    ef.allPoints.push_back(efp);
    ef.nPoints++;
    phs.push_back(ph);
    return ph;
  }
  // PointFrameResidual + EnergyFunctional::insertResidual (:445-458)
  PointFrameResidual* addResidual(PointHessian* ph, int target_idx, int id) {
    PointFrameResidual* pfr = new PointFrameResidual;
    pfr->point = ph; pfr->host = ph->host; pfr->target = fhs[target_idx]; pfr->id = id;
    EFResidual* efr = new EFResidual{pfr, effs[target_idx]};
    efr->point = ph->efPoint; efr->idxInAll = (int)ph->efPoint->residualsAll.size();
    pfr->efResidual = efr;
    ph->efPoint->residualsAll.push_back(efr);
    ph->residuals.push_back(pfr);
    ef.nResiduals++;
    return pfr;
  }
  void build(const std::string& dir, const Options& o) {
    meta = load<int>(dir, "meta");
    nf = meta[0]; np = meta[1]; nr = meta[2]; w = meta[3]; h = meta[4];
    calib = load<double>(dir, "calib");
    auto evalPT = load<double>(dir, "evalPT"), state = load<double>(dir, "state"), state_zero = load<double>(dir, "state_zero");
    auto exposure = load<float>(dir, "ab_exposure"), eTH = load<float>(dir, "frameEnergyTH");
    auto frameID = load<int>(dir, "frameID"), res_point = load<int>(dir, "res_point"), res_target = load<int>(dir, "res_target");
    host = load<int>(dir, "host");
    auto u = load<float>(dir, "u"), v = load<float>(dir, "v"), idepth = load<float>(dir, "idepth"), idz = load<float>(dir, "idepth_zero"),
         color = load<float>(dir, "color"), weights = load<float>(dir, "weights");
    auto prior = load<uint8_t>(dir, "hasDepthPrior"), res_state = load<uint8_t>(dir, "res_state");
    std::vector<float> mrb; std::vector<int> ngood; std::vector<uint8_t> isnew;
    if (o.extras) { mrb = load<float>(dir, "maxRelBaseline"); ngood = load<int>(dir, "numGoodResiduals"); isnew = load<uint8_t>(dir, "res_isNew"); }
    const int n_files = o.frames_on_file ? o.frames_on_file : nf;
    for (int f = 0; f < n_files; f++) {
      FrameHessian* fh = new FrameHessian;
      fhs.push_back(fh);
      load_pyramid(dir, "img" + std::to_string(f), *fh, o.levels);
      fh->slot = 10 + f;
      if (f >= (int)frameID.size()) break;
      fh->worldToCam_evalPT = se3_of(&evalPT[f * 12]);
      for (int i = 0; i < 10; i++) { fh->state[i] = state[f * 10 + i]; fh->state_zero[i] = state_zero[f * 10 + i]; }
      fh->affFromState = true;
      fh->ab_exposure = exposure[f]; fh->frameEnergyTH = eTH[f]; fh->frameID = frameID[f]; fh->idx = f; fh->shell->id = 100 + f;
      effs.push_back(new EFFrame{fh, {}, f});
      fh->efFrame = effs.back();
      if (f < nf) ef.frames.push_back(effs.back());
    }
    int r = 0;
    for (int p = 0; p < np; p++) {
      PointHessian* ph = addPoint(host[p]);
      ph->u = u[p]; ph->v = v[p]; ph->idepth = idepth[p]; ph->idepth_zero = idz[p]; ph->hasDepthPrior = prior[p] != 0;
      if (o.extras) { ph->maxRelBaseline = mrb[p]; ph->numGoodResiduals = ngood[p]; }
      for (int k = 0; k < 8; k++) { ph->color[k] = color[p * 8 + k]; ph->weights[k] = weights[p * 8 + k]; }
      for (; r < nr && res_point[r] == p; r++) {
        PointFrameResidual* pfr = addResidual(ph, res_target[r], r);
        pfr->state_state = (ResState)res_state[r];
        if (o.extras) pfr->isNew = isnew[r] != 0;
        pfrs.push_back(pfr);
        // lastResiduals: [0] the residual into the newest frame, [1] into the one before (FullSystem.cpp:1400-1410)
        const int k = nf - 1 - res_target[r];
        if (k == 0 || k == 1) ph->lastResiduals[k] = {pfr, o.last_state_from_file ? (ResState)res_state[r] : IN};
      }
      if (o.point_hessians) fhs[host[p]]->pointHessians.push_back(ph);
    }
    if (o.swap_a >= 0) {
      if (host[o.swap_a] != host[o.swap_b]) throw std::runtime_error("the two swapped points must share their host");
      auto& l = fhs[host[o.swap_a]]->pointHessians;
      std::swap(*std::find(l.begin(), l.end(), phs[o.swap_a]), *std::find(l.begin(), l.end(), phs[o.swap_b]));
    }
    const int n = 8 * nf + 4;
    ef.HM.resize(n, n); ef.bM.assign(n, 0.0);
    if (o.extras) { ef.HM.d = load<double>(dir, "HM"); ef.bM = load<double>(dir, "bM"); }
    for (int i = 0; i < 4; i++) { HC.value_scaled[i] = calib[i]; HC.value_zero[i] = calib[4 + i]; }
  }
  WindowGraph() {}
  WindowGraph(const WindowGraph&) = delete;
  ~WindowGraph() {
    for (PointHessian* ph : phs) {
      for (PointFrameResidual* pfr : ph->residuals) { delete pfr->efResidual; delete pfr; }
      delete ph->efPoint;
      delete ph;
    }
    for (EFFrame* f : effs) delete f;
    for (FrameHessian* fh : fhs) delete fh;
  }
};
