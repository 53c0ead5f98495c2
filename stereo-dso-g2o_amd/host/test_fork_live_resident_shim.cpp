// sdso_shim::optimizeForkLiveResident and the pair optimizeForkLiveBegin / optimizeForkLiveEnd (host/fork_live.h) — FullSystem::optimize as
// the fork compiles it, FullSystemOptimize.cpp:402-868, with the loop's controller resident on the device — on stand-ins for the
// reference's types, next to the C-ABI call on the same window.  tests/test_g2o_lba_resident_shim_gpu.py writes the window as raw arrays,
// runs this program and compares what the routes leave:
//   abi    the graph flattened here by hand, sdso_g2o_lba_optimize_resident; the estimates and per-residual results as they come back
//   shim   optimizeForkLiveResident on a graph of its own; every member the write-back of :682-727 touches, per frame, residual, point
//   split  optimizeForkLiveBegin, host work (an unrelated frame is uploaded, sdso_g2o_lba_optimize_done is polled once, a sum is formed),
//          optimizeForkLiveEnd on a third graph; the same members
// activeResiduals is every residual of the window in file order, as in test_fork_live_shim.cpp.
//
//   test_fork_live_resident_shim <dir>     files: those of test_fork_live_shim
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

// every member the write-back touches, under `pre`
static void dump_graph(const std::string& dir, const std::string& pre, const WindowGraph& B, float rmse) {
  const int nf = B.nf, nr = B.nr;
  std::vector<double> cal(16), twh((size_t)nf * 12), thw((size_t)nf * 12), st((size_t)nf * 4);
  for (int i = 0; i < 4; i++) {
    cal[i] = B.HC.value[i]; cal[4 + i] = B.HC.value_scaled[i]; cal[8 + i] = B.HC.value_scaledf[i]; cal[12 + i] = B.HC.value_minus_value_zero[i];
  }
  std::vector<float> cali(4);
  for (int i = 0; i < 4; i++) cali[i] = B.HC.value_scaledi[i];
  for (int f = 0; f < nf; f++) {
    const FrameHessian* fh = B.fhs[f];
    for (int k = 0; k < 9; k++) { twh[f * 12 + k] = fh->PRE_camToWorld.R.m[k]; thw[f * 12 + k] = fh->PRE_worldToCam.R.m[k]; }
    for (int k = 0; k < 3; k++) { twh[f * 12 + 9 + k] = fh->PRE_camToWorld.t[k]; thw[f * 12 + 9 + k] = fh->PRE_worldToCam.t[k]; }
    st[f * 4] = fh->state[6]; st[f * 4 + 1] = fh->state[7]; st[f * 4 + 2] = fh->state_scaled[6]; st[f * 4 + 3] = fh->state_scaled[7];
  }
  std::vector<float> cpt((size_t)nr * 3);
  std::vector<double> en((size_t)nr * 2);
  std::vector<uint8_t> ns(nr);
  for (int r = 0; r < nr; r++) {
    const PointFrameResidual* p = B.pfrs[r];
    for (int k = 0; k < 3; k++) cpt[(size_t)r * 3 + k] = p->centerProjectedTo[k];
    en[r * 2] = p->state_NewEnergy; en[r * 2 + 1] = p->state_NewEnergyWithOutlier; ns[r] = (uint8_t)p->state_NewState;
  }
  std::vector<float> pt((size_t)B.np * 5);
  for (int p = 0; p < B.np; p++) {
    const PointHessian* ph = B.phs[p];
    pt[p * 5] = ph->idepth; pt[p * 5 + 1] = ph->idepth_scaled; pt[p * 5 + 2] = ph->idepth_zero; pt[p * 5 + 3] = ph->idepth_hessian; pt[p * 5 + 4] = ph->efPoint->HdiF;
  }
  dump(dir, (pre + "_calib").c_str(), cal); dump(dir, (pre + "_calib_i").c_str(), cali); dump(dir, (pre + "_Twh").c_str(), twh); dump(dir, (pre + "_Thw").c_str(), thw);
  dump(dir, (pre + "_state").c_str(), st); dump(dir, (pre + "_cpt").c_str(), cpt); dump(dir, (pre + "_energy").c_str(), en); dump(dir, (pre + "_newstate").c_str(), ns);
  dump(dir, (pre + "_points").c_str(), pt); dump(dir, (pre + "_rmse").c_str(), &rmse, 1);
  std::printf("%s: rmse %.6f\n", pre.c_str(), rmse);
}

static void prepare(WindowGraph& G, const std::string& dir) {
  WindowGraph::Options o;
  G.build(dir, o);
  auto Twh = load<double>(dir, "Twh"), Ttw = load<double>(dir, "Ttw");
  for (int f = 0; f < G.nf; f++) {
    G.fhs[f]->PRE_camToWorld = se3_of(&Twh[f * 12]);
    G.fhs[f]->PRE_worldToCam = se3_of(&Ttw[f * 12]);
  }
  for (PointHessian* ph : G.phs) { ph->idepth_scaled = ph->idepth; ph->idepth_hessian = 7.0f; }   // a value the call must replace or keep, visibly
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const int iterations = load<int>(dir, "iterations")[0];
  try {
    sdso_shim::Device dev(0);
    WindowGraph A, B, C;
    prepare(A, dir);
    prepare(B, dir);
    prepare(C, dir);
    const int nf = A.nf, nr = A.nr;
    const int lv = 1, w[1] = {A.w}, h[1] = {A.h};
    for (int f = 0; f < nf; f++) dev.uploadFrame(A.fhs[f]->slot, A.fhs[f], lv, w, h);
    // ---- abi
    {
      std::vector<int> slot(nf), host(nr), target(nr);
      std::vector<sdso_se3_t> Ttw(nf), Twh(nf);
      std::vector<sdso_aff_t> taff(nf), haff(nf);
      std::vector<float> ex(nf), eth(nf), u(nr), v(nr), col((size_t)nr * 8), wgt((size_t)nr * 8);
      std::vector<double> b0(nf), idepth(nr);
      for (int f = 0; f < nf; f++) {
        FrameHessian* fh = A.fhs[f];
        slot[f] = fh->slot; Ttw[f] = sdso_shim::toAbi(fh->PRE_worldToCam); Twh[f] = sdso_shim::toAbi(fh->PRE_camToWorld);
        taff[f] = haff[f] = sdso_aff_t{fh->aff_g2l().a, fh->aff_g2l().b};
        b0[f] = fh->aff_g2l().b; ex[f] = fh->ab_exposure; eth[f] = fh->frameEnergyTH;
      }
      for (int r = 0; r < nr; r++) {
        PointFrameResidual* p = A.pfrs[r];
        host[r] = p->host->idx; target[r] = p->target->idx; u[r] = p->point->u; v[r] = p->point->v; idepth[r] = p->point->idepth;
        for (int k = 0; k < 8; k++) { col[(size_t)r * 8 + k] = p->point->color[k]; wgt[(size_t)r * 8 + k] = p->point->weights[k]; }
      }
      sdso_g2o_lba_window_t W = {nf, nr, A.w, A.h, slot.data(), Ttw.data(), taff.data(), ex.data(), b0.data(), eth.data(), host.data(), target.data(),
                                 u.data(), v.data(), col.data(), wgt.data()};
      sdso_g2o_lba_state_t S = {Twh.data(), haff.data(), {A.HC.fxl(), A.HC.fyl(), A.HC.cxl(), A.HC.cyl()}, idepth.data()};
      const sdso_g2o_lba_opt_t P = {iterations, 0.1, 1e-3, 10};
      std::vector<uint8_t> st(nr), lvl(nr), act(nr);
      std::vector<float> en((size_t)nr * 2), cpt((size_t)nr * 3), ih(nr);
      sdso_g2o_lba_result_t out = {};
      out.state = st.data(); out.energy = en.data(); out.centerProjectedTo = cpt.data(); out.edge_level = lvl.data(); out.idepth_hessian = ih.data();
      out.active = act.data();
      dev.check(sdso_g2o_lba_optimize_resident(dev.ctx(), &W, &P, &S, &out), "sdso_g2o_lba_optimize_resident");
      std::vector<double> twh((size_t)nf * 12), aff((size_t)nf * 2);
      for (int f = 0; f < nf; f++) {
        for (int k = 0; k < 9; k++) twh[f * 12 + k] = Twh[f].R[k];
        for (int k = 0; k < 3; k++) twh[f * 12 + 9 + k] = Twh[f].t[k];
        aff[f * 2] = haff[f].a; aff[f * 2 + 1] = haff[f].b;
      }
      dump(dir, "abi_Twh", twh); dump(dir, "abi_aff", aff); dump(dir, "abi_cam", S.cam, 4); dump(dir, "abi_idepth", idepth);
      dump(dir, "abi_state", st); dump(dir, "abi_energy", en); dump(dir, "abi_cpt", cpt); dump(dir, "abi_ih", ih); dump(dir, "abi_active", act);
      const float rmse = out.rmse;
      const int scal[3] = {out.iterations, out.stop, out.n_active};
      dump(dir, "abi_rmse", &rmse, 1); dump(dir, "abi_scalars", scal, 3);
      std::printf("abi: iterations %d stop %d n_active %d rmse %.6f\n", out.iterations, out.stop, out.n_active, rmse);
    }
    // ---- shim
    {
      std::vector<PointFrameResidual*> activeResiduals = B.pfrs;
      std::vector<FrameHessian*> frameHessians(B.fhs.begin(), B.fhs.begin() + nf);
      const float rmse = sdso_shim::optimizeForkLiveResident(dev, frameHessians, activeResiduals, B.HC, [](const FrameHessian* fh) { return fh->slot; }, iterations, B.w, B.h);
      dump_graph(dir, "shim", B, rmse);
    }
    // ---- split: host work between enqueue and write-back
    {
      std::vector<PointFrameResidual*> activeResiduals = C.pfrs;
      std::vector<FrameHessian*> frameHessians(C.fhs.begin(), C.fhs.begin() + nf);
      sdso_shim::ForkLiveJob job = sdso_shim::optimizeForkLiveBegin(dev, frameHessians, activeResiduals, C.HC, [](const FrameHessian* fh) { return fh->slot; }, iterations, C.w, C.h);
      const int done_early = sdso_g2o_lba_optimize_done(dev.ctx());
      dev.uploadFrame(900, C.fhs[0], lv, w, h);                    // an unrelated slot
      double work = 0;
      for (const PointHessian* ph : C.phs) work += ph->idepth;      // reads nothing the write-back touches later
      const float rmse = sdso_shim::optimizeForkLiveEnd(dev, job, activeResiduals, C.HC);
      const int after[2] = {done_early, sdso_g2o_lba_optimize_done(dev.ctx())};
      dump(dir, "split_done", after, 2);
      std::printf("split: done polled %d, after the fetch %d, host work %.3f\n", after[0], after[1], work);
      dump_graph(dir, "split", C, rmse);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
