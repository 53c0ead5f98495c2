// Keyframe steps through sdso_shim::WindowedBA::update on stand-ins for the reference's types.  tests/test_window_update_shim_gpu.py writes
// the window as raw arrays, runs this program and compares what it leaves (out_*.bin) with the same steps through the C-ABI from Python.
//   step 1  upload, FullSystem::optimize (the shim drops linearizeAll(true)'s toRemove from the EnergyFunctional), removeOutliers (points
//           left without a residual are flagged PS_DROP, ef->dropPointsF()), update() instead of a second upload
//   step 2  (when s2_* files exist) insertFrame, insertResidual into it, insertPoint with residuals, update(): the window grows by a frame
//   step 3  marginalizePointsF on the grown window, the removePoint loop with willRemovePoint, WindowedBA::marginalizeFrame of the oldest
//           frame, the residual drops of FullSystem::marginalizeFrame, update()
//
//   test_window_update <dir>
#include <map>
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
static void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
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
struct Vec3f { float v[3]; };
struct Vec10 { double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct VecC { double v[4] = {0, 0, 0, 0}; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct Vec2f { float v[2] = {0, 0}; float& operator[](int i) { return v[i]; } };
struct Vec3fv { float v[3] = {0, 0, 0}; float& operator[](int i) { return v[i]; } };
struct CalibHessian {
  VecC value_scaled, value_zero, value, step;
  void setValue(const VecC& val) { value = val; for (int i = 0; i < 4; i++) value_scaled[i] = 50.0 * val[i]; }   // HessianBlocks.h:318-333 (SCALE_F = SCALE_C = 50)
};
struct FrameHessian {
  Vec3f* dIp[SDSO_PYR_LEVELS];
  std::vector<float> store;
  SE3 worldToCam_evalPT; Vec10 state, state_zero, step;
  float ab_exposure = 1, frameEnergyTH = 0; int frameID = 0, slot = 0;
  const SE3& get_worldToCam_evalPT() const { return worldToCam_evalPT; }
  const Vec10& get_state() const { return state; }
  const Vec10& get_state_zero() const { return state_zero; }
  void setState(const Vec10& s) { state = s; }
  void setEvalPT(const SE3& T, const Vec10& s) { worldToCam_evalPT = T; state = s; state_zero = s; }
};
struct EFFrame; struct EFPoint; struct EFResidual; struct PointHessian;
struct PointFrameResidual {
  int state_state = 0, state_NewState = 0;
  double state_energy = 0, state_NewEnergy = 0, state_NewEnergyWithOutlier = 0;
  bool isNew = true;
  Vec2f projectedTo[SDSO_MAX_RES];
  Vec3fv centerProjectedTo;
  PointHessian* point = nullptr; EFResidual* efResidual = nullptr;
  int id = -1;                                                   // index in the uploaded window (the test's bookkeeping)
};
struct PointHessian {
  float u, v, idepth, idepth_zero, color[8], weights[8], step = 0, idepth_hessian = 0, maxRelBaseline = 0;
  int numGoodResiduals = 0;
  bool hasDepthPrior = false;
  std::vector<PointFrameResidual*> residuals;
  std::pair<PointFrameResidual*, int> lastResiduals[2] = {{nullptr, 2}, {nullptr, 2}};
  EFPoint* efPoint = nullptr;
  int id = -1;
  void setIdepth(float x) { idepth = x; }
  void setIdepthZero(float x) { idepth_zero = x; }
};
enum { PS_GOOD = 0, PS_MARGINALIZE = 1, PS_DROP = 2 };           // EFPointStatus
struct EFResidual { PointFrameResidual* data; EFFrame* target; bool isActiveAndIsGoodNEW = false; int idxInAll = 0; EFPoint* point = nullptr; bool isLinearized = false; };
struct EFPoint { PointHessian* data; std::vector<EFResidual*> residualsAll; int stateFlag = PS_GOOD; float HdiF = 0, bdSumF = 0, deltaF = 0; int idxInPoints = 0; EFFrame* host = nullptr; };
struct EFFrame { FrameHessian* data; std::vector<EFPoint*> points; int idx; };
struct DynMat {
  int n = 0; std::vector<double> d;
  void resize(int r, int c) { n = c; d.assign((size_t)r * c, 0.0); }
  double& operator()(int i, int j) { return d[(size_t)i * n + j]; }
};
struct DynVec {
  std::vector<double> d;
  void resize(int r) { d.assign((size_t)r, 0.0); }
  double& operator()(int i) { return d[(size_t)i]; }
};
// what std::vector-based lists of the reference do when an entry leaves: the last entry takes its slot (and learns its new index)
template <class T, class SetIdx>
static void swap_out(std::vector<T*>& list, int idx, SetIdx set_idx) {
  list[idx] = list.back();
  set_idx(list[idx], idx);
  list.pop_back();
}
struct EnergyFunctional {
  std::vector<EFFrame*> frames; DynMat HM, lastHS; std::vector<double> bM, lastbS, lastX;
  int resInA = 0, resInL = 0, resInM = 0, nResiduals = 0, nPoints = 0;
  void dropResidual(EFResidual* r) {                             // semantics of EnergyFunctional.cpp:524-551
    swap_out(r->point->residualsAll, r->idxInAll, [](EFResidual* moved, int k) { moved->idxInAll = k; });
    r->data->efResidual = nullptr;
    nResiduals--;
    delete r;
  }
  void removePoint(EFPoint* p) {                                 // semantics of :755-772: the point's residuals go, then the point leaves its host's list
    while (!p->residualsAll.empty()) {
      PointFrameResidual* pfr = p->residualsAll.back()->data;
      dropResidual(p->residualsAll.back());
      delete pfr;
    }
    p->data->residuals.clear();
    swap_out(p->host->points, p->idxInPoints, [](EFPoint* moved, int k) { moved->idxInPoints = k; });
    p->data->efPoint = nullptr;
    nPoints--;
    delete p;
  }
  void dropPointsF() {                                           // semantics of :739-752: a slot is looked at again after a removal filled it
    for (EFFrame* f : frames) {
      size_t at = 0;
      while (at < f->points.size()) {
        if (f->points[at]->stateFlag == PS_DROP) removePoint(f->points[at]);
        else at++;
      }
    }
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_window_update <dir>\n"); return 2; }
  const std::string dir = argv[1];
  try {
    sdso_shim::Device dev(0);
    auto meta = load<int>(dir, "meta");                          // nf np nr w h its solverMode
    const int nf = meta[0], np = meta[1], nr = meta[2], w = meta[3], h = meta[4];
    const int nf_all = meta.size() > 7 ? meta[7] : nf;             // frames on file; the first nf make the uploaded window
    auto calib = load<double>(dir, "calib");                     // value_scaled(4) value_zero(4)
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
    int wv[1] = {w}, hv[1] = {h};
    for (int f = 0; f < nf_all; f++) {
      fhs.emplace_back(new FrameHessian);
      FrameHessian& fh = *fhs.back();
      char nm[32]; std::snprintf(nm, sizeof nm, "img%d_l0", f);
      fh.store = load<float>(dir, nm);
      fh.dIp[0] = reinterpret_cast<Vec3f*>(fh.store.data());
      for (int i = 0; i < 9; i++) fh.worldToCam_evalPT.R.m[i] = evalPT[f * 12 + i];
      for (int i = 0; i < 3; i++) fh.worldToCam_evalPT.t.v[i] = evalPT[f * 12 + 9 + i];
      for (int i = 0; i < 10; i++) { fh.state[i] = state[f * 10 + i]; fh.state_zero[i] = state_zero[f * 10 + i]; }
      fh.ab_exposure = exposure[f]; fh.frameEnergyTH = eTH[f]; fh.frameID = frameID[f]; fh.slot = 10 + f;
      dev.uploadFrame(fh.slot, &fh, 1, wv, hv);
      effs.emplace_back(new EFFrame{&fh, {}, f});
      if (f < nf) ef.frames.push_back(effs.back().get());
    }
    int r = 0;
    for (int p = 0; p < np; p++) {
      phs.emplace_back(new PointHessian);
      PointHessian& ph = *phs.back();
      ph.u = u[p]; ph.v = v[p]; ph.idepth = idepth[p]; ph.idepth_zero = idz[p]; ph.hasDepthPrior = prior[p] != 0; ph.id = p;
      for (int k = 0; k < 8; k++) { ph.color[k] = color[p * 8 + k]; ph.weights[k] = weights[p * 8 + k]; }
      EFPoint* efp = new EFPoint{&ph, {}, PS_GOOD};             // raw new: the reference deletes what it removes
      efp->host = effs[host[p]].get(); efp->idxInPoints = (int)efp->host->points.size();
      ph.efPoint = efp;
      for (; r < nr && res_point[r] == p; r++) {
        PointFrameResidual* pfr = new PointFrameResidual;
        pfr->state_state = (int)res_state[r]; pfr->point = &ph; pfr->id = r;
        EFResidual* efr = new EFResidual{pfr, effs[res_target[r]].get()};
        efr->point = efp; efr->idxInAll = (int)efp->residualsAll.size();
        pfr->efResidual = efr;
        efp->residualsAll.push_back(efr);
        ph.residuals.push_back(pfr);
        ef.nResiduals++;
      }
      efp->host->points.push_back(efp);
      ef.nPoints++;
    }
    const int n = 8 * nf + 4;
    ef.HM.resize(n, n); ef.bM.assign(n, 0.0);
    for (int i = 0; i < 4; i++) { HC.value_scaled[i] = calib[i]; HC.value_zero[i] = calib[4 + i]; }

    sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, 0);
    ba.upload(&ef, &HC, w, h, /*solverMode=*/meta[6], 1e12, 1e8, true, [](FrameHessian* fh) { return fh->slot; });
    ba.optimize(meta[5], &ef, &HC);                              // drops toRemove from the EnergyFunctional (and notes it for update())
    // removeOutliers (FullSystem.cpp: points without a residual are flagged PS_DROP, then ef->dropPointsF())
    int dropped = 0;
    for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) if (p->residualsAll.empty()) { p->stateFlag = PS_DROP; dropped++; }
    ba.willDropPoints([](EFPoint* p) { return p->stateFlag == PS_DROP; });
    ef.dropPointsF();
    ba.update(&ef, [](FrameHessian* fh) { return fh->slot; });
    std::printf("removed %d dropped %d nResiduals %d nPoints %d\n", ba.lastRemoved, dropped, ef.nResiduals, ef.nPoints);

    // ---- what the edited window holds and computes
    std::vector<int> o_points, o_res;                            // the EnergyFunctional's order as ids of the original window
    for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) { o_points.push_back(p->data->id); for (EFResidual* er : p->residualsAll) o_res.push_back(er->data->id); }
    std::vector<int> g_frames(nf), g_points(ef.nPoints), g_res(ef.nResiduals);
    dev.check(sdso_ba_window_get_order(dev.ctx(), 0, g_frames.data(), g_points.data(), g_res.data()), "sdso_ba_window_get_order");
    std::vector<double> o_state(nf * 10);
    std::vector<float> o_idepth(ef.nPoints);
    std::vector<uint8_t> o_rstate(ef.nResiduals);
    dev.check(sdso_ba_get_state(dev.ctx(), 0, o_state.data(), o_idepth.data(), o_rstate.data()), "sdso_ba_get_state");
    std::vector<double> o_energy = {ba.linearizeAll()};
    ba.applyRes(); ba.accumulateAll();
    DynMat H3[3]; DynVec b3[3];
    ba.accumulateAF_MT(H3[0], b3[0], false); ba.accumulateLF_MT(H3[1], b3[1], false); ba.accumulateSCF_MT(H3[2], b3[2], false);
    std::vector<double> o_st;
    for (int k = 0; k < 3; k++) { o_st.insert(o_st.end(), H3[k].d.begin(), H3[k].d.end()); o_st.insert(o_st.end(), b3[k].d.begin(), b3[k].d.end()); }
    dump(dir, "ef_points", o_points); dump(dir, "ef_res", o_res); dump(dir, "order_points", g_points); dump(dir, "order_res", g_res);
    dump(dir, "state", o_state); dump(dir, "idepth", o_idepth); dump(dir, "rstate", o_rstate); dump(dir, "energy", o_energy); dump(dir, "stitched", o_st);
    if (std::ifstream(dir + "/s2_pt_host.bin")) {
      auto slot_of = [](FrameHessian* fh) { return fh->slot; };
      auto walk = [&](std::vector<int>& pts, std::vector<int>& res) {
        pts.clear(); res.clear();
        for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) { pts.push_back(p->data->id); for (EFResidual* er : p->residualsAll) res.push_back(er->data->id); }
      };
      auto add_residual = [&](PointHessian& ph, EFFrame* target, int id) {      // PointFrameResidual + EnergyFunctional::insertResidual (:445-458)
        PointFrameResidual* pfr = new PointFrameResidual;
        pfr->point = &ph; pfr->id = id;
        EFResidual* efr = new EFResidual{pfr, target};
        efr->point = ph.efPoint; efr->idxInAll = (int)ph.efPoint->residualsAll.size();
        pfr->efResidual = efr;
        ph.efPoint->residualsAll.push_back(efr);
        ph.residuals.push_back(pfr);
        ef.nResiduals++;
      };
      std::map<int, EFPoint*> by_id;
      for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) by_id[p->data->id] = p;
      // ---- step 2: insertFrame (:462-504: HM / bM grow by a zero block), insertResidual, insertPoint (:507-521)
      EFFrame* fresh = effs[nf].get();
      fresh->idx = (int)ef.frames.size();
      ef.frames.push_back(fresh);
      int n2 = 8 * (int)ef.frames.size() + 4;
      ef.HM.resize(n2, n2); ef.bM.assign(n2, 0.0);
      auto ar_point = load<int>(dir, "s2_add_res_point");
      int next_res = nr;
      for (int id : ar_point) add_residual(*by_id.at(id)->data, fresh, next_res++);
      auto pt_host = load<int>(dir, "s2_pt_host"), pr_point = load<int>(dir, "s2_pr_point"), pr_target = load<int>(dir, "s2_pr_target");
      auto pt_u = load<float>(dir, "s2_pt_u"), pt_v = load<float>(dir, "s2_pt_v"), pt_id = load<float>(dir, "s2_pt_idepth"), pt_col = load<float>(dir, "s2_pt_color"),
           pt_w = load<float>(dir, "s2_pt_weights");
      size_t k = 0;
      for (size_t q = 0; q < pt_host.size(); q++) {
        phs.emplace_back(new PointHessian);
        PointHessian& ph = *phs.back();
        ph.u = pt_u[q]; ph.v = pt_v[q]; ph.idepth = ph.idepth_zero = pt_id[q]; ph.id = np + (int)q;
        for (int c = 0; c < 8; c++) { ph.color[c] = pt_col[q * 8 + c]; ph.weights[c] = pt_w[q * 8 + c]; }
        EFPoint* efp = new EFPoint{&ph, {}, PS_GOOD};
        efp->host = effs[pt_host[q]].get(); efp->idxInPoints = (int)efp->host->points.size();
        ph.efPoint = efp;
        efp->host->points.push_back(efp);
        ef.nPoints++;
        for (; k < pr_point.size() && pr_point[k] == (int)q; k++) add_residual(ph, effs[pr_target[k]].get(), next_res++);
      }
      ba.update(&ef, slot_of);
      std::vector<int> e_pts, e_res;
      walk(e_pts, e_res);
      dump(dir, "s2_ef_points", e_pts); dump(dir, "s2_ef_res", e_res);
      // ---- step 3: marginalizePointsF (the prior now has the grown window's dimension), the removePoint loop, marginalizeFrame
      auto marg_ids = load<int>(dir, "s3_marg");
      by_id.clear();
      for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) by_id[p->data->id] = p;
      for (int id : marg_ids) by_id.at(id)->stateFlag = PS_MARGINALIZE;
      ba.marginalizePointsF(&ef, [](EFPoint* p) { return p->stateFlag == PS_MARGINALIZE; });
      dump(dir, "s3_HM", ef.HM.d); dump(dir, "s3_bM", ef.bM);
      std::vector<EFPoint*> allPointsToMarg;
      for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) if (p->stateFlag == PS_MARGINALIZE) allPointsToMarg.push_back(p);
      for (EFPoint* p : allPointsToMarg) { ba.willRemovePoint(p); ef.removePoint(p); }
      EFFrame* oldest = ef.frames[0];
      ba.marginalizeFrame(&ef, oldest);
      dump(dir, "s3_HMf", ef.HM.d); dump(dir, "s3_bMf", ef.bM);
      for (EFFrame* f : ef.frames)                                    // FullSystem::marginalizeFrame (FullSystemMarginalize.cpp:150-180): residuals into the frame go
        for (EFPoint* p : f->points)
          for (size_t i = 0; i < p->residualsAll.size(); i++)
            if (p->residualsAll[i]->target == oldest) {
              PointFrameResidual* pfr = p->residualsAll[i]->data;
              auto& rl = p->data->residuals;
              rl.erase(std::find(rl.begin(), rl.end(), pfr));
              ef.dropResidual(p->residualsAll[i]);
              delete pfr;
              break;
            }
      ef.frames.erase(ef.frames.begin());
      for (size_t i = 0; i < ef.frames.size(); i++) ef.frames[i]->idx = (int)i;
      ba.update(&ef, slot_of);
      walk(e_pts, e_res);
      dump(dir, "s3_ef_points", e_pts); dump(dir, "s3_ef_res", e_res);
      std::vector<double> s_state(ef.frames.size() * 10), s_energy;
      std::vector<float> s_idepth(ef.nPoints);
      std::vector<uint8_t> s_rstate(ef.nResiduals);
      dev.check(sdso_ba_get_state(dev.ctx(), 0, s_state.data(), s_idepth.data(), s_rstate.data()), "sdso_ba_get_state");
      s_energy.push_back(ba.linearizeAll());
      ba.applyRes(); ba.accumulateAll();
      DynMat S3[3]; DynVec c3[3];
      ba.accumulateAF_MT(S3[0], c3[0], false); ba.accumulateLF_MT(S3[1], c3[1], false); ba.accumulateSCF_MT(S3[2], c3[2], false);
      std::vector<double> s_st;
      for (int q = 0; q < 3; q++) { s_st.insert(s_st.end(), S3[q].d.begin(), S3[q].d.end()); s_st.insert(s_st.end(), c3[q].d.begin(), c3[q].d.end()); }
      dump(dir, "s3_idepth", s_idepth); dump(dir, "s3_rstate", s_rstate); dump(dir, "s3_energy", s_energy); dump(dir, "s3_stitched", s_st);
      std::printf("step 3: nf %d nPoints %d nResiduals %d\n", (int)ef.frames.size(), ef.nPoints, ef.nResiduals);
    }
    // the graph's leftovers
    for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) { for (EFResidual* er : p->residualsAll) { delete er->data; delete er; } delete p; }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_window_update: %s\n", e.what());
    return 1;
  }
  return 0;
}
