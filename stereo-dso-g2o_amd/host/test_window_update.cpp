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
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_window_update <dir>\n"); return 2; }
  const std::string dir = argv[1];
  try {
    sdso_shim::Device dev(0);
    const auto m = load<int>(dir, "meta");                         // nf np nr w h its solverMode [frames on file; the first nf make the uploaded window]
    WindowGraph G;
    WindowGraph::Options opt;
    if (m.size() > 7) opt.frames_on_file = m[7];
    G.build(dir, opt);
    const int nf = G.nf, np = G.np, nr = G.nr, w = G.w, h = G.h;
    auto& meta = G.meta; EnergyFunctional& ef = G.ef; CalibHessian& HC = G.HC;
    int wv[1] = {w}, hv[1] = {h};
    for (FrameHessian* fh : G.fhs) dev.uploadFrame(fh->slot, fh, 1, wv, hv);

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
    MatXX H3[3]; VecX b3[3];
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
      std::map<int, EFPoint*> by_id;
      for (EFFrame* f : ef.frames) for (EFPoint* p : f->points) by_id[p->data->id] = p;
      // ---- step 2: insertFrame (:462-504: HM / bM grow by a zero block), insertResidual, insertPoint (:507-521)
      EFFrame* fresh = G.effs[nf];
      fresh->idx = (int)ef.frames.size();
      ef.frames.push_back(fresh);
      int n2 = 8 * (int)ef.frames.size() + 4;
      ef.HM.resize(n2, n2); ef.bM.assign(n2, 0.0);
      auto ar_point = load<int>(dir, "s2_add_res_point");
      int next_res = nr;
      for (int id : ar_point) G.addResidual(by_id.at(id)->data, nf, next_res++);
      auto pt_host = load<int>(dir, "s2_pt_host"), pr_point = load<int>(dir, "s2_pr_point"), pr_target = load<int>(dir, "s2_pr_target");
      auto pt_u = load<float>(dir, "s2_pt_u"), pt_v = load<float>(dir, "s2_pt_v"), pt_id = load<float>(dir, "s2_pt_idepth"), pt_col = load<float>(dir, "s2_pt_color"),
           pt_w = load<float>(dir, "s2_pt_weights");
      size_t k = 0;
      for (size_t q = 0; q < pt_host.size(); q++) {
        PointHessian& ph = *G.addPoint(pt_host[q]);                    // its id is np + q
        ph.u = pt_u[q]; ph.v = pt_v[q]; ph.idepth = ph.idepth_zero = pt_id[q];
        for (int c = 0; c < 8; c++) { ph.color[c] = pt_col[q * 8 + c]; ph.weights[c] = pt_w[q * 8 + c]; }
        for (; k < pr_point.size() && pr_point[k] == (int)q; k++) G.addResidual(&ph, pr_target[k], next_res++);
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
      MatXX S3[3]; VecX c3[3];
      ba.accumulateAF_MT(S3[0], c3[0], false); ba.accumulateLF_MT(S3[1], c3[1], false); ba.accumulateSCF_MT(S3[2], c3[2], false);
      std::vector<double> s_st;
      for (int q = 0; q < 3; q++) { s_st.insert(s_st.end(), S3[q].d.begin(), S3[q].d.end()); s_st.insert(s_st.end(), c3[q].d.begin(), c3[q].d.end()); }
      dump(dir, "s3_idepth", s_idepth); dump(dir, "s3_rstate", s_rstate); dump(dir, "s3_energy", s_energy); dump(dir, "s3_stitched", s_st);
      std::printf("step 3: nf %d nPoints %d nResiduals %d\n", (int)ef.frames.size(), ef.nPoints, ef.nResiduals);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_window_update: %s\n", e.what());
    return 1;
  }
  return 0;
}
