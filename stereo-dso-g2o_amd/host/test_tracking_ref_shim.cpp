// sdso_shim::CoarseTracker::setCoarseTrackingRef on the device-resident window against the overload that walks the pointer graph, on
// stand-ins for the reference's types.  tests/test_tracking_ref_shim_gpu.py writes a window as raw arrays and runs this program twice:
//   test_tracking_ref_shim <dir> window   WindowedBA::writeBackProjections = false, optimize, setCoarseTrackingRef(ba, frameHessians, fh_right)
//   test_tracking_ref_shim <dir> graph    the full write-back, optimize, setCoarseTrackingRef(frameHessians, fh_right, Hcalib)
// and compares the template levels each run leaves (out_<mode>_*.bin) bit for bit.  FrameHessian::pointHessians of one host is NOT in
// the window's point order (two entries swapped, meta[8..9]): the splat order is pointHessians order in both runs.
#include <cstdio>
#include "sdso_shim.h"
#include "driver_io.h"

using Tracker = sdso_shim::CoarseTracker<SE3, AffLight, Mat33, Vec3>;

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: test_tracking_ref_shim <dir> window|graph\n"); return 2; }
  const std::string dir = argv[1], mode = argv[2];
  const bool from_window = mode == "window";
  if (!from_window && mode != "graph") { std::fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
  try {
    sdso_shim::Device dev(0);
    const auto m = load<int>(dir, "meta");                         // nf np nr w h its solverMode levels swapA swapB
    const int levels = m[7];
    WindowGraph G;                                                 // calib = value_scaled(4) value_zero(4) baseline
    WindowGraph::Options opt;
    opt.levels = levels; opt.frames_on_file = m[0] + 1;            // frame nf on file: the right image of the newest keyframe
    opt.last_state_from_file = true; opt.point_hessians = true; opt.swap_a = m[8]; opt.swap_b = m[9];
    G.build(dir, opt);
    const int nf = G.nf, w = G.w, h = G.h;
    auto& meta = G.meta; auto& calib = G.calib; auto& fhs = G.fhs; auto& phs = G.phs; EnergyFunctional& ef = G.ef; CalibHessian& HC = G.HC;
    std::vector<int> wv(levels), hv(levels);
    for (int l = 0; l < levels; l++) { wv[l] = w >> l; hv[l] = h >> l; }
    for (FrameHessian* fh : fhs) dev.uploadFrame(fh->slot, fh, levels, wv.data(), hv.data());
    auto slot_of_fh = [](FrameHessian* fh) { return fh->slot; };

    sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, 0);
    ba.writeBackProjections = !from_window;
    ba.upload(&ef, &HC, w, h, /*solverMode=*/meta[6], 1e12, 1e8, true, slot_of_fh);
    ba.optimize(meta[5], &ef, &HC);
    int cpt_written = 0;                                         // residual objects whose centerProjectedTo the optimize call filled
    for (auto& ph : phs) for (PointFrameResidual* pfr : ph->residuals) cpt_written += pfr->centerProjectedTo[2] != 0.f;

    std::vector<FrameHessian*> frameHessians;
    for (int f = 0; f < nf; f++) frameHessians.push_back(fhs[f]);
    FrameHessian* fh_right = fhs[nf];
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
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_tracking_ref_shim: %s\n", e.what());
    return 1;
  }
  return 0;
}
