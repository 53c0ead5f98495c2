// Driver for sdso_shim::CoarseDistanceMap, selectPointsToActivate and updateMinActDist on stand-in types that carry the reference's
// member names (Eigen / Sophus are not available here).  tests/test_distmap_shim_gpu.py writes the inputs as raw arrays, runs this
// program and compares what it dumps with the C-ABI path; `minact` needs no device.
//   test_distmap_shim minact <current> <desired> n1 n2 ...      one line per n: currentMinActDist after STEP 1
//   test_distmap_shim run <dir>                                 makeK, makeDistanceMap, addIntoDistFinal, STEP 2
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "sdso_shim.h"

template <class T>
static std::vector<T> load(const std::string& dir, const char* name) {
  std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
  if (!f) { std::fprintf(stderr, "missing %s\n", name); std::exit(2); }
  f.seekg(0, std::ios::end);
  const size_t bytes = (size_t)f.tellg();
  f.seekg(0);
  std::vector<T> v(bytes / sizeof(T));
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}
template <class T>
static void dump(const std::string& dir, const char* name, const T* p, size_t n) {
  std::ofstream f(dir + "/out_" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

struct Mat33 { double m[9]; double& operator()(int i, int j) { return m[i * 3 + j]; } double operator()(int i, int j) const { return m[i * 3 + j]; } };
struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct Mat33f { float m[9]; float& operator()(int i, int j) { return m[i * 3 + j]; } float operator()(int i, int j) const { return m[i * 3 + j]; } };
struct SE3 {
  Mat33 R; Vec3 t;
  const Mat33& rotationMatrix() const { return R; }
  const Vec3& translation() const { return t; }
  SE3 operator*(const SE3& o) const {
    SE3 r;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) r.R(i, j) = (R(i, 0) * o.R(0, j) + R(i, 1) * o.R(1, j)) + R(i, 2) * o.R(2, j);
      r.t[i] = ((R(i, 0) * o.t[0] + R(i, 1) * o.t[1]) + R(i, 2) * o.t[2]) + t[i];
    }
    return r;
  }
};
struct CalibHessian {
  float f[4];
  float fxl() const { return f[0]; } float fyl() const { return f[1]; } float cxl() const { return f[2]; } float cyl() const { return f[3]; }
};
struct FrameHessian;
struct PointHessian { float u, v, idepth_scaled; };
struct ImmaturePoint {
  float u, v, idepth_min, idepth_max, quality, lastTracePixelInterval, my_type;
  int lastTraceStatus;
  FrameHessian* host;
  int idxInImmaturePoints = -1;
  int id;                       // position in the flattened input, to report the outcome
};
struct FrameHessian {
  SE3 PRE_worldToCam, PRE_camToWorld;
  bool flaggedForMarginalization = false;
  std::vector<PointHessian*> pointHessians;
  std::vector<ImmaturePoint*> immaturePoints;
};

static SE3 se3_of(const double* p) {
  SE3 T;
  for (int i = 0; i < 9; i++) T.R.m[i] = p[i];
  for (int i = 0; i < 3; i++) T.t[i] = p[9 + i];
  return T;
}

static int run(const std::string& dir) {
  const auto meta = load<int>(dir, "meta");   // w h levels nf
  const int w = meta[0], h = meta[1], levels = meta[2], nf = meta[3];
  const auto calib = load<float>(dir, "calib");
  const auto w2c = load<double>(dir, "worldToCam"), c2w = load<double>(dir, "camToWorld");
  const auto flagged = load<uint8_t>(dir, "flagged");
  const auto a_host = load<int>(dir, "a_host");
  const auto a_u = load<float>(dir, "a_u"), a_v = load<float>(dir, "a_v"), a_id = load<float>(dir, "a_idepth");
  const auto c_host = load<int>(dir, "c_host"), c_st = load<int>(dir, "c_status");
  const auto c_u = load<float>(dir, "c_u"), c_v = load<float>(dir, "c_v"), c_min = load<float>(dir, "c_idepth_min"), c_max = load<float>(dir, "c_idepth_max"),
             c_q = load<float>(dir, "c_quality"), c_itv = load<float>(dir, "c_interval"), c_ty = load<float>(dir, "c_my_type");
  const auto par = load<float>(dir, "par");   // currentMinActDist, setting_minTraceQuality
  const auto add = load<int>(dir, "add");     // pairs (u, v)

  std::vector<FrameHessian> frames(nf);
  std::vector<FrameHessian*> frameHessians;
  for (int f = 0; f < nf; f++) {
    frames[f].PRE_worldToCam = se3_of(&w2c[12 * f]);
    frames[f].PRE_camToWorld = se3_of(&c2w[12 * f]);
    frames[f].flaggedForMarginalization = f < nf - 1 && flagged[f] != 0;
    frameHessians.push_back(&frames[f]);
  }
  std::vector<PointHessian> phs(a_u.size());
  for (size_t i = 0; i < a_u.size(); i++) { phs[i] = PointHessian{a_u[i], a_v[i], a_id[i]}; frames[a_host[i]].pointHessians.push_back(&phs[i]); }
  const int nc = (int)c_u.size();
  std::vector<ImmaturePoint*> all(nc);
  for (int i = 0; i < nc; i++) {
    all[i] = new ImmaturePoint{c_u[i], c_v[i], c_min[i], c_max[i], c_q[i], c_itv[i], c_ty[i], c_st[i], &frames[c_host[i]], -1, i};
    frames[c_host[i]].immaturePoints.push_back(all[i]);
  }

  sdso_shim::Device dev(0);
  sdso_shim::CoarseDistanceMap<Mat33f> cdm(dev, w, h);
  CalibHessian Hcalib{{calib[0], calib[1], calib[2], calib[3]}};
  cdm.makeK(&Hcalib, levels, w, h);
  const size_t npix = (size_t)cdm.w[1] * cdm.h[1];
  std::vector<sdso_distmap_geom_t> geoms;
  for (int f = 0; f < nf - 1; f++) geoms.push_back(cdm.geomOf(&frames[f], &frames[nf - 1]));
  dump(dir, "geoms", reinterpret_cast<const float*>(geoms.data()), geoms.size() * 12);

  cdm.makeDistanceMap(frameHessians, &frames[nf - 1]);
  dump(dir, "map0", cdm.distFinal(), npix);
  const int numItems = cdm.numItems;
  for (size_t i = 0; i + 1 < add.size(); i += 2) cdm.addIntoDistFinal(add[i], add[i + 1]);
  dump(dir, "map1", cdm.distFinal(), npix);

  cdm.makeDistanceMap(frameHessians, &frames[nf - 1]);
  // the deleted candidates are gone after the call: remember who sits where first
  std::vector<std::vector<int>> ids(nf);
  for (int f = 0; f < nf; f++) for (auto* p : frames[f].immaturePoints) ids[f].push_back(p->id);
  std::vector<ImmaturePoint*> toOptimize = sdso_shim::selectPointsToActivate(cdm, frameHessians, par[0], par[1]);
  std::vector<uint8_t> decision(nc, 0);
  std::vector<int> order;
  for (int f = 0; f < nf; f++)
    for (size_t i = 0; i < frames[f].immaturePoints.size(); i++) {
      ImmaturePoint* p = frames[f].immaturePoints[i];
      if (p == 0) decision[ids[f][i]] = 1;
      else if (f < nf - 1 && p->idxInImmaturePoints != (int)i) { std::fprintf(stderr, "idxInImmaturePoints not set\n"); return 1; }
    }
  for (auto* p : toOptimize) { decision[p->id] = 2; order.push_back(p->id); }
  dump(dir, "decision", decision.data(), decision.size());
  dump(dir, "order", order.data(), order.size());
  dump(dir, "map2", cdm.distFinal(), npix);
  std::printf("numItems %d toOptimize %d\n", numItems, (int)toOptimize.size());
  for (int f = 0; f < nf; f++) for (auto* p : frames[f].immaturePoints) delete p;
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "minact")) {
    for (int i = 4; i < argc; i++) {
      float c = (float)std::atof(argv[2]);
      sdso_shim::updateMinActDist(c, std::atoi(argv[i]), (float)std::atof(argv[3]));
      std::printf("%.9g\n", c);
    }
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "run")) {
    try { return run(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  std::fprintf(stderr, "usage: test_distmap_shim minact <current> <desired> n... | run <dir>\n");
  return 2;
}
