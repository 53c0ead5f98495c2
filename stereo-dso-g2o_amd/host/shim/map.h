#pragma once
#include <algorithm>
#include <map>
#include "device.h"
#include "marshal.h"
namespace sdso_shim {
// ---- The device-resident map (sdso_map_*): what FullSystem::makeKeyFrame publishes through publishKeyframes (FullSystem.cpp:1467,
// FullSystemMarginalize.cpp:184) and KeyFrameDisplay turns into vertices and colours.
//
// PointMap::update(ba, frameHessians) — setFromKF's copy of every keyframe's three PointHessian lists, made on the device while the
// window's post-state is valid: call it after ba.flagPointsForRemoval(frameHessians) and before marginalizePointsF / ba.update().
//   active : each frame's pointHessians as the two functions compacted them
//   gone   : the tail each frame's pointHessiansOut / pointHessiansMarginalized has grown by since the previous call (the two sizes are
//            kept per frameID), which is the reference's push order.  A keyframe that joins with lists already filled: note(fh) first,
//            after sdso_map_put of what they hold.
// frameHessians: std::vector<FrameHessian*>-like in window order; of a frame frameID and the three lists are read.  Throws Error when the
// device refuses, and then keeps its sizes as they were.
class PointMap {
 public:
  explicit PointMap(Device& dev) : dev_(dev) {}
  template <class WindowedBAT, class FrameHessians> void update(WindowedBAT& ba, FrameHessians& frameHessians) {
    std::vector<int> active, gone;
    std::vector<uint8_t> gone_list;
    std::map<int, Sizes> now = sizes_;
    auto index = [&](const auto* ph) {
      const int i = ph->efPoint ? ba.pointIndexOf(ph->efPoint) : -1;
      if (i < 0) throw Error("PointMap::update: a listed point is not part of the device window (call it before dropPointsF / update())");
      return i;
    };
    for (auto* fh : frameHessians) {
      for (auto* ph : fh->pointHessians) active.push_back(index(ph));
      Sizes& s = now[fh->frameID];
      if (s.out > fh->pointHessiansOut.size() || s.marg > fh->pointHessiansMarginalized.size()) throw Error("PointMap::update: a list of a known frame shrank");
      for (size_t k = s.out; k < fh->pointHessiansOut.size(); k++) { gone.push_back(index(fh->pointHessiansOut[k])); gone_list.push_back(3); }
      for (size_t k = s.marg; k < fh->pointHessiansMarginalized.size(); k++) { gone.push_back(index(fh->pointHessiansMarginalized[k])); gone_list.push_back(2); }
      s.out = fh->pointHessiansOut.size(); s.marg = fh->pointHessiansMarginalized.size();
    }
    sdso_map_update_t U;
    U.n_active = (int)active.size(); U.active = active.data();
    U.n_gone = (int)gone.size(); U.gone = gone.data(); U.gone_list = gone_list.data();
    dev_.check(sdso_map_update(dev_.ctx(), ba.win(), &U), "sdso_map_update");
    sizes_.swap(now);
  }
  template <class FrameHessianT> void note(const FrameHessianT* fh) { sizes_[fh->frameID] = Sizes{fh->pointHessiansOut.size(), fh->pointHessiansMarginalized.size()}; }
  // after the frame's `final = true` publication (FullSystemMarginalize.cpp:184)
  void release(int frameID) { dev_.check(sdso_map_release_keyframe(dev_.ctx(), frameID), "sdso_map_release_keyframe"); sizes_.erase(frameID); }
  // records (16 floats each, sdso_abi.h) of list 1 (active), 2 (marginalised) or 3 (out) of a keyframe
  std::vector<float> records(int frameID, int list) const {
    int c[3] = {0, 0, 0};
    dev_.check(sdso_map_counts(dev_.ctx(), frameID, c), "sdso_map_counts");
    std::vector<float> r((size_t)c[list - 1] * 16);
    dev_.check(sdso_map_get(dev_.ctx(), frameID, list, r.data()), "sdso_map_get");
    return r;
  }

 private:
  struct Sizes { size_t out = 0, marg = 0; };
  Device& dev_;
  std::map<int, Sizes> sizes_;
};
// KeyFrameDisplay (IOWrapper/Pangolin/KeyFrameDisplay.h) on the map, with the reference's member names and signatures.
//   setFromKF(fh, HCalib)   notes the frameID, the immature group (immGroupOf(fh), -1: none; with sdso_shim::ImmaturePoints it is the
//                           frame's slot), the calibration and PRE_camToWorld; sets needRefresh (:85-165).  The points themselves stay
//                           in the map: a refresh reads the lists as they are then, which is what the reference shows too, since every
//                           publishKeyframes calls setFromKF first.
//   refreshPC(...)          the reference's needRefresh logic and return values (:176-200, :297-302, :322): false when nothing had to be
//                           done or the keyframe has no point, true after a rebuild — with no vertex the buffers stay as they were.
//   vertices() / colors() / numGLBufferGoodPoints stand for the two GL buffers: 3 floats and 3 bytes per vertex, camera frame (the
//                           reference's buffer; camToWorld is the member the caller puts into the GL matrix).  vertices_dev / colors_dev of
//                           the latest refresh of ANY display: sdso_map_cloud_dev.
//   refreshPC(displays, ..) the many-frames form: one sdso_map_cloud per 8 displays that need a refresh — a whole publishKeyframes call.
// Deviations (sdso_abi.h): no z jitter, and sparsity != 1 throws Error — both draw rand() in the reference.
template <class FrameHessianT, class CalibHessianT> class KeyFrameDisplay {
 public:
  using SE3T = typename std::decay<decltype(std::declval<FrameHessianT>().PRE_camToWorld)>::type;
  KeyFrameDisplay(Device& dev, std::function<int(const FrameHessianT*)> immGroupOf = nullptr) : dev_(dev), imm_group_of_(std::move(immGroupOf)) {}
  int id = 0;                                                  // KeyFrameDisplay.h:91-93
  bool active = true;
  SE3T camToWorld;
  int numGLBufferGoodPoints = 0;                               // :118
  bool bufferValid = false;                                    // :116

  void setFromKF(FrameHessianT* fh, CalibHessianT* HCalib) {
    id = fh->shell->id;                                        // setFromF (:70-82)
    detail::calibK4(*HCalib, K4_);
    frameID_ = fh->frameID;
    imm_group_ = imm_group_of_ ? imm_group_of_(fh) : -1;
    camToWorld = fh->PRE_camToWorld;                           // :163
    needRefresh = true;                                        // :164
    set_ = true;
  }
  bool refreshPC(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    std::vector<KeyFrameDisplay*> one{this};
    return refreshPC(one, canRefresh, scaledTH, absTH, mode, minBS, sparsity)[0];
  }
  static std::vector<bool> refreshPC(const std::vector<KeyFrameDisplay*>& displays, bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    if (sparsity != 1) throw Error("KeyFrameDisplay::refreshPC: sparsity != 1 draws rand() in the reference and is not built");
    std::vector<bool> ret(displays.size(), false);
    std::vector<size_t> todo;
    size_t at = 0;
    try {
    for (size_t i = 0; i < displays.size(); i++)
      if (displays[i]->begin_(canRefresh, scaledTH, absTH, mode, minBS, sparsity)) todo.push_back(i);
    for (; at < todo.size(); at += 8) {
      const int n = (int)std::min<size_t>(8, todo.size() - at);
      KeyFrameDisplay& d0 = *displays[todo[at]];
      int fid[8], imm[8], first[9];
      long bound = 0;
      for (int k = 0; k < n; k++) {
        KeyFrameDisplay& d = *displays[todo[at + k]];
        if (&d.dev_ != &d0.dev_ || !std::equal(d.K4_, d.K4_ + 4, d0.K4_)) throw Error("KeyFrameDisplay::refreshPC: the displays of one call share the device and the calibration");
        fid[k] = d.frameID_; imm[k] = d.imm_group_; bound += d.numSparsePoints_;
      }
      std::vector<float> xyz((size_t)bound * 8 * 3);
      std::vector<uint8_t> rgb((size_t)bound * 8 * 3);
      sdso_map_cloud_t Q;
      Q.n_frames = n; Q.frameID = fid; Q.imm_host_id = imm;
      Q.fx = d0.K4_[0]; Q.fy = d0.K4_[1]; Q.cx = d0.K4_[2]; Q.cy = d0.K4_[3];
      Q.scaledTH = scaledTH; Q.absTH = absTH; Q.minBS = minBS; Q.mode = mode;
      Q.camToWorld = nullptr; Q.cap = (int)(bound * 8);
      d0.dev_.check(sdso_map_cloud(d0.dev_.ctx(), &Q, xyz.data(), rgb.data(), first, nullptr), "sdso_map_cloud");
      for (int k = 0; k < n; k++) {
        KeyFrameDisplay& d = *displays[todo[at + k]];
        ret[todo[at + k]] = true;
        const int nv = first[k + 1] - first[k];
        if (nv == 0) continue;                                 // :297-302: the buffers stay as they were
        d.numGLBufferGoodPoints = nv;                          // :304
        d.vertices_.assign(xyz.begin() + (size_t)first[k] * 3, xyz.begin() + (size_t)first[k + 1] * 3);
        d.colors_.assign(rgb.begin() + (size_t)first[k] * 3, rgb.begin() + (size_t)first[k + 1] * 3);
        d.bufferValid = true;                                  // :317
      }
    }
    } catch (...) {                                            // begin_() cleared needRefresh on displays whose buffers were not rebuilt
      for (size_t k = at; k < todo.size(); k++) displays[todo[k]]->needRefresh = true;
      throw;
    }
    return ret;
  }
  const std::vector<float>& vertices() const { return vertices_; }      // numGLBufferGoodPoints * 3
  const std::vector<uint8_t>& colors() const { return colors_; }

 private:
  // :176-200 up to "make data": true when the points have to be rebuilt
  bool begin_(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity) {
    if (!set_) throw Error("KeyFrameDisplay::refreshPC: setFromKF first");
    if (canRefresh)
      needRefresh = needRefresh || my_scaledTH != scaledTH || my_absTH != absTH || my_displayMode != mode || my_minRelBS != minBS || my_sparsifyFactor != sparsity;
    if (!needRefresh) return false;
    int c[3] = {0, 0, 0}, ni = 0;                              // (asked first: a refusal leaves needRefresh set)
    dev_.check(sdso_map_counts(dev_.ctx(), frameID_, c), "sdso_map_counts");
    if (imm_group_ >= 0) dev_.check(sdso_imm_count(dev_.ctx(), imm_group_, &ni), "sdso_imm_count");
    needRefresh = false;
    my_scaledTH = scaledTH; my_absTH = absTH; my_displayMode = mode; my_minRelBS = minBS; my_sparsifyFactor = sparsity;
    numSparsePoints_ = ni + c[0] + c[1] + c[2];                // :90-93
    return numSparsePoints_ != 0;                              // :199-200
  }
  Device& dev_;
  std::function<int(const FrameHessianT*)> imm_group_of_;
  float K4_[4] = {0, 0, 0, 0};
  bool needRefresh = true, set_ = false;                       // :57-67
  float my_scaledTH = 1e10f, my_absTH = 1e10f, my_minRelBS = 0;
  int my_displayMode = 1, my_sparsifyFactor = 1;
  int frameID_ = -1, imm_group_ = -1, numSparsePoints_ = 0;
  std::vector<float> vertices_;
  std::vector<uint8_t> colors_;
};
}  // namespace sdso_shim
