// The threaded binding of INTEGRATION.md §2 with a device buffer pool: the schedule of test_handoff_shim.cpp (a mapping thread on one
// sdso_shim::Device builds a template per keyframe and exports it with the frames the tracker wants, a tracking thread on another Device
// adopts and imports them) with ONE sdso_shim::Pool attached to both Devices (Device::setPool), so that the frames and templates of
// keyframe k + 1 are built in the buffers keyframe k - 1 left behind while the other thread may still be reading them.
//   test_pool_shim <dir>    <dir>/k<k>/ holds window k (K = meta[0] of <dir>/meta.bin, the files of WindowGraph in every k<k>)
// runs the schedule on two Devices and two threads under the pool, then on ONE Device in one thread without a pool, dumps both (out_two /
// out_one: per tracked frame 12 pose doubles, 2 affine, 5 lastResiduals, 5 iteration counts, refFrameID, good) and the pool's counters
// (out_stats: hits misses frees host_waits overflow_waits parked_buffers parked_bytes), and exits 0 only if the runs are bit-equal and
// the pool made no host wait.
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include "sdso_shim.h"
#include "driver_io.h"

using Tracker = sdso_shim::CoarseTracker<SE3, AffLight, Mat33, Vec3>;
constexpr int kTracked = 3, kRec = 26;

struct Post {                          // what makeKeyFrame leaves for the tracking thread, and deliverTrackedFrame's frames the other way round
  int k = -1;
  Tracker::TrackingRef ref;
  sdso_shim::Shared frame[kTracked];
  float exposure[kTracked] = {0, 0, 0};
  double K[4] = {0, 0, 0, 0};
  int w = 0, h = 0, levels = 0;
};

// makeKeyFrame's part: window k up, optimised, its template built from the resident window and exported; the frames the tracker will
// want exported too; then everything of keyframe k is released on the mapper's Device — the blocks live on with their other holders
static Post map_keyframe(sdso_shim::Device& dev, Tracker& trk, const std::string& dir, int k, int its) {
  const std::string kd = dir + "/k" + std::to_string(k);
  const auto m = load<int>(kd, "meta");                          // nf np nr w h its solverMode levels
  const int levels = m[7];
  WindowGraph G;
  WindowGraph::Options opt;
  opt.levels = levels; opt.frames_on_file = m[0] + 1;            // frame nf on file: the right image of the newest keyframe
  opt.last_state_from_file = true; opt.point_hessians = true;
  G.build(kd, opt);
  const int nf = G.nf, w = G.w, h = G.h;
  std::vector<int> wv(levels), hv(levels);
  for (int l = 0; l < levels; l++) { wv[l] = w >> l; hv[l] = h >> l; }
  for (size_t f = 0; f < G.fhs.size(); f++) {
    G.fhs[f]->slot = 100 * (k % 2) + 10 + (int)f;                // two sets of slots taken in turn
    G.fhs[f]->shell->id = 1000 * k + 100 + (int)f;
    dev.uploadFrame(G.fhs[f]->slot, G.fhs[f], levels, wv.data(), hv.data());
  }
  sdso_shim::WindowedBA<EnergyFunctional, CalibHessian> ba(dev, /*win=*/k % 2);
  ba.writeBackProjections = false;
  ba.upload(&G.ef, &G.HC, w, h, /*solverMode=*/G.meta[6], 1e12, 1e8, true, [](FrameHessian* fh) { return fh->slot; });
  ba.optimize(its, &G.ef, &G.HC);
  std::vector<FrameHessian*> frameHessians(G.fhs.begin(), G.fhs.begin() + nf);
  trk.baseline = (float)G.calib[8];
  trk.setCoarseTrackingRef(ba, frameHessians, G.fhs[nf]);
  Post p;
  p.k = k; p.w = w; p.h = h; p.levels = levels;
  p.ref = trk.exportRef();
  for (int j = 0; j < kTracked; j++) {
    FrameHessian* fh = G.fhs[nf - 2 - j];
    p.frame[j] = dev.exportFrame(fh->slot);
    p.exposure[j] = fh->ab_exposure;
  }
  for (int i = 0; i < 4; i++) p.K[i] = G.HC.value_scaled[i];
  dev.check(sdso_ba_release_window(dev.ctx(), ba.win()), "sdso_ba_release_window");
  for (FrameHessian* fh : G.fhs) dev.releaseFrame(fh->slot);
  return p;                                                      // (G goes: ref.lastRef is a name from here on, as a culled FrameHessian* would be)
}

// the tracking thread's part: the swap, then kTracked frames against template k
static void track_keyframe(sdso_shim::Device& dev, Tracker& trk, Post& p, int nf, std::vector<double>& out) {
  trk.adoptRef(p.ref);
  if (trk.refFrameID != 1000 * p.k + 100 + nf - 1) throw sdso_shim::Error("refFrameID does not follow the keyframe");
  if (trk.firstCoarseRMSE != -1 || trk.params().ref_exposure != p.ref.ab_exposure || trk.params().ref_aff_g2l.a != p.ref.lastRef_aff_g2l.a ||
      trk.params().ref_aff_g2l.b != p.ref.lastRef_aff_g2l.b)
    throw sdso_shim::Error("adoptRef did not run the bookkeeping of a new reference");
  CalibHessian HC;
  for (int i = 0; i < 4; i++) HC.value_scaled[i] = p.K[i];
  trk.makeK(&HC, p.levels, p.w, p.h);
  p.ref = Tracker::TrackingRef();                                // the handle goes; the tracker's slot holds the template
  for (int j = 0; j < kTracked; j++) {
    const int slot = 50 + j;
    dev.importFrame(slot, p.frame[j]);
    p.frame[j] = sdso_shim::Shared();
    SE3 T; AffLight aff;
    Vec5 minRes; for (int i = 0; i < 5; i++) minRes.v[i] = NAN;
    const bool good = trk.trackNewestCoarse(slot, p.exposure[j], T, aff, p.levels - 1, minRes);
    for (int i = 0; i < 9; i++) out.push_back(T.R.m[i]);
    for (int i = 0; i < 3; i++) out.push_back(T.t[i]);
    out.push_back(aff.a); out.push_back(aff.b);
    for (int i = 0; i < 5; i++) out.push_back(trk.lastResiduals[i]);
    for (int i = 0; i < 5; i++) out.push_back((double)trk.lastStats.iterations[i]);
    out.push_back((double)trk.refFrameID); out.push_back(good ? 1.0 : 0.0);
  }
}

struct Mailbox {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Post> q;
  bool closed = false;
  std::string error;
  void put(Post&& p) { { std::lock_guard<std::mutex> g(mu); q.push_back(std::move(p)); } cv.notify_all(); }
  void close(const std::string& err) { { std::lock_guard<std::mutex> g(mu); closed = true; if (error.empty()) error = err; } cv.notify_all(); }
  bool take(Post& p) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !q.empty() || closed; });
    if (q.empty()) return false;
    p = std::move(q.front()); q.pop_front();
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_pool_shim <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const auto top = load<int>(dir, "meta");                       // K nf its
  const int K = top[0], nf = top[1], its = top[2];
  std::vector<double> two, one;
  sdso_pool_stats_t st{};
  try {
    {   // ---- two Devices, two threads, one pool
      sdso_shim::Pool pool(0);
      {
        sdso_shim::Device gpuMap(0), gpuTrack(0);
        gpuMap.setPool(pool); gpuTrack.setPool(pool);
        Tracker forNewKF(gpuMap, /*ref_slot=*/1), tracker(gpuTrack, /*ref_slot=*/2);
        forNewKF.slot_of = [](const void* fh) { return static_cast<const FrameHessian*>(fh)->slot; };
        Mailbox box;
        std::thread mapper([&] {
          try {
            for (int k = 0; k < K; k++) box.put(map_keyframe(gpuMap, forNewKF, dir, k, its));
            box.close("");
          } catch (const std::exception& e) { box.close(std::string("mapper: ") + e.what()); }
        });
        std::thread tracking([&] {
          try {
            Post p;
            while (box.take(p)) track_keyframe(gpuTrack, tracker, p, nf, two);
          } catch (const std::exception& e) { box.close(std::string("tracker: ") + e.what()); }
        });
        mapper.join();
        tracking.join();
        if (!box.error.empty()) throw sdso_shim::Error(box.error);
      }
      st = pool.stats();                                           // both Devices are gone: what they held is parked
      pool.trim(0);
      if (pool.stats().parked_bytes != 0) throw sdso_shim::Error("trim left completed buffers parked");
    }
    {   // ---- the same schedule on one Device, one thread, no pool
      sdso_shim::Device gpu(0);
      Tracker forNewKF(gpu, 1), tracker(gpu, 2);
      forNewKF.slot_of = [](const void* fh) { return static_cast<const FrameHessian*>(fh)->slot; };
      for (int k = 0; k < K; k++) {
        Post p = map_keyframe(gpu, forNewKF, dir, k, its);
        track_keyframe(gpu, tracker, p, nf, one);
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_pool_shim: %s\n", e.what());
    return 1;
  }
  dump(dir, "two", two);
  dump(dir, "one", one);
  const std::vector<double> stats = {(double)st.hits, (double)st.misses, (double)st.frees, (double)st.host_waits, (double)st.overflow_waits,
                                     (double)st.parked_buffers, (double)st.parked_bytes};
  dump(dir, "stats", stats);
  if (two.size() != (size_t)K * kTracked * kRec || one.size() != two.size()) { std::fprintf(stderr, "test_pool_shim: %zu / %zu results\n", two.size(), one.size()); return 1; }
  if (std::memcmp(two.data(), one.data(), sizeof(double) * two.size()) != 0) { std::fprintf(stderr, "test_pool_shim: the two runs differ\n"); return 1; }
  if (st.host_waits != 0 || st.overflow_waits != 0) { std::fprintf(stderr, "test_pool_shim: %lld host waits\n", st.host_waits); return 1; }
  if (st.hits <= 0 || st.misses != st.frees + st.parked_buffers) { std::fprintf(stderr, "test_pool_shim: hits %lld misses %lld frees %lld parked %lld\n", st.hits, st.misses, st.frees, st.parked_buffers); return 1; }
  std::printf("pool ok: %d keyframes, %d tracked frames, bit-equal under a pool on two Devices / two threads and without one on one; hits %lld misses %lld host_waits %lld\n",
              K, K * kTracked, st.hits, st.misses, st.host_waits);
  return 0;
}
