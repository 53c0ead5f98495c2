// sdso_shim::optimizeForkLive (host/fork_live.h) — FullSystem::optimize as the fork compiles it, FullSystemOptimize.cpp:402-868 — on
// stand-ins for the reference's types, next to the C-ABI call on the same window.  tests/test_g2o_lba_shim_gpu.py writes the window as
// raw arrays, runs this program and compares what the two routes leave:
//   abi    the graph flattened here by hand, sdso_g2o_lba_optimize; the estimates and per-residual results are dumped as they come back
//   shim   optimizeForkLive on a graph of its own; every member the write-back of :682-727 touches is dumped, per frame, residual, point
// activeResiduals is every residual of the window in file order (grouped by point: a point's residuals follow each other, so "the last
// residual of a point wins" is visible).
//
//   test_fork_live_shim <dir>     files: those of WindowGraph, and Twh (nf x 12: PRE_camToWorld), Ttw (nf x 12: PRE_worldToCam), iterations (1 int)
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

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
    WindowGraph A, B;
    prepare(A, dir);
    prepare(B, dir);
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
      dev.check(sdso_g2o_lba_optimize(dev.ctx(), &W, &P, &S, &out), "sdso_g2o_lba_optimize");
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
      const float rmse = sdso_shim::optimizeForkLive(dev, frameHessians, activeResiduals, B.HC, [](const FrameHessian* fh) { return fh->slot; }, iterations, B.w, B.h);
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
      dump(dir, "shim_calib", cal); dump(dir, "shim_calib_i", cali); dump(dir, "shim_Twh", twh); dump(dir, "shim_Thw", thw); dump(dir, "shim_state", st);
      dump(dir, "shim_cpt", cpt); dump(dir, "shim_energy", en); dump(dir, "shim_newstate", ns); dump(dir, "shim_points", pt); dump(dir, "shim_rmse", &rmse, 1);
      std::printf("shim: rmse %.6f\n", rmse);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
