// Stand-ins for the reference's types, for the test drivers of sdso_shim.h (neither Eigen nor Sophus exists here).  Every type carries the
// reference's name and, of its members, the ones some driver touches, each with the header and line it mirrors (src/ of the reference:
// util/NumType.h, util/FrameShell.h, util/MinimalImage.h, FullSystem/HessianBlocks.h, FullSystem/Residuals.h, FullSystem/ImmaturePoint.h,
// OptimizationBackend/EnergyFunctionalStructs.h, OptimizationBackend/EnergyFunctional.h).  This file is the one statement of what the
// shim expects from those types.  It includes the ABI header for two constants and nothing of the shim, so a program can use it without
// the device library.  Members marked "test:" are the drivers' bookkeeping, not the reference's.
//
// What must NOT be added, because the shim selects an overload on it: an inverse() on the 3x3 types (detail::inverse33), a constructor
// that makes ImmaturePoint not default-constructible (detail::newImmaturePoint).
#pragma once
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>
#include "../../include/sdso_abi.h"

// ---- util/NumType.h: fixed-size Eigen vectors / matrices, row-major here, zero where Eigen leaves them uninitialised
template <class S, int N> struct Vec_ {
  S v[N] = {};
  S& operator[](int i) { return v[i]; }
  S operator[](int i) const { return v[i]; }
};
template <class S, int R, int C> struct Mat_ {
  S m[R * C] = {};
  S& operator()(int i, int j) { return m[i * C + j]; }
  S operator()(int i, int j) const { return m[i * C + j]; }
};
using Mat33 = Mat_<double, 3, 3>;   // NumType.h:63
using Mat88 = Mat_<double, 8, 8>;   // :70
using VecC = Vec_<double, 4>;       // :73 (CPARS = 4)
using Vec10 = Vec_<double, 10>;     // :76
using Vec8 = Vec_<double, 8>;       // :78
using Vec5 = Vec_<double, 5>;       // :81
using Vec3 = Vec_<double, 3>;       // :83
using Vec2 = Vec_<double, 2>;       // :84
using Mat33f = Mat_<float, 3, 3>;   // :87
using Mat22f = Mat_<float, 2, 2>;   // :89
using Vec3f = Vec_<float, 3>;       // :90; also the {I, dx, dy} pixel of FrameHessian::dIp (12 bytes, no padding)
using Vec2f = Vec_<float, 2>;       // :91
using Mat18f = Mat_<float, 1, 8>;   // :115
using Mat88f = Mat_<float, 8, 8>;   // :117
using Vector2i = Vec_<int, 2>;      // Eigen::Vector2i (util/Undistort.h getSize / getOriginalSize)
struct MatXX {                      // :49
  int n = 0; std::vector<double> d;
  void resize(int r, int c) { n = c; d.assign((size_t)r * c, 0.0); }
  double& operator()(int i, int j) { return d[(size_t)i * n + j]; }
};
struct VecX {                       // :85
  std::vector<double> d;
  void resize(int r) { d.assign((size_t)r, 0.0); }
  double& operator()(int i) { return d[(size_t)i]; }
  double& operator[](int i) { return d[(size_t)i]; }
};
struct SE3 {                        // :42 (Sophus::SE3d): identity by default, (R, t), product
  Mat33 R; Vec3 t;
  SE3() { for (int i = 0; i < 3; i++) R(i, i) = 1; }
  SE3(const Mat33& R_, const Vec3& t_) : R(R_), t(t_) {}
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
  SE3 inverse() const {             // Sophus se3.hpp:169: (R^T, -R^T t)
    SE3 r;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.R(i, j) = R(j, i);
    for (int i = 0; i < 3; i++) r.t[i] = -((r.R(i, 0) * t[0] + r.R(i, 1) * t[1]) + r.R(i, 2) * t[2]);
    return r;
  }
};
struct AffLight {                   // :152-175
  double a = 0, b = 0;
  static Vec2 fromToVecExposure(float exposureF, float exposureT, AffLight g2F, AffLight g2T) {   // :159-167
    if (exposureF == 0 || exposureT == 0) exposureT = exposureF = 1;
    const double a = std::exp(g2T.a - g2F.a) * exposureT / exposureF;
    return Vec2{{a, g2T.b - a * g2F.b}};
  }
};
struct FrameShell { int id = 0; };                                  // util/FrameShell.h:38
template <class T> struct MinimalImage { int w, h; T* data; };      // util/MinimalImage.h:35-37

struct FrameHessian; struct PointHessian; struct ImmaturePoint; struct PointFrameResidual;
struct EFFrame; struct EFPoint; struct EFResidual;

// ---- FullSystem/HessianBlocks.h
struct FrameFramePrecalc { Mat33f PRE_RTll; Vec2f PRE_aff_mode; Vec3f PRE_tTll; };   // :80, :85, :88
struct CalibHessian {
  VecC value_zero, value_scaled, value, step;                       // :276-281
  Vec_<float, 4> value_scaledf, value_scaledi;                      // :278-279 (VecCf); written by the fork-live optimize only: fxl() .. cyl() below read value_scaled
  VecC value_minus_value_zero;                                      // :284
  CalibHessian() {}
  CalibHessian(float fx, float fy, float cx, float cy) { value_scaled[0] = fx; value_scaled[1] = fy; value_scaled[2] = cx; value_scaled[3] = cy; }   // test: floats survive the double
  void setValue(const VecC& val) {                                  // :318-333 (SCALE_F = SCALE_C = 50)
    value = val;
    for (int i = 0; i < 4; i++) value_scaled[i] = 50.0 * val[i];
  }
  float fxl() const { return (float)value_scaled[0]; }              // :307-310 (value_scaledf)
  float fyl() const { return (float)value_scaled[1]; }
  float cxl() const { return (float)value_scaled[2]; }
  float cyl() const { return (float)value_scaled[3]; }
};
struct FrameHessian {
  FrameShell* shell = &shellStore;                                  // :105
  Vec3f* dIp[SDSO_PYR_LEVELS] = {};                                 // :108
  EFFrame* efFrame = nullptr;                                       // :101
  int frameID = 0, idx = -1;                                        // :111, :113
  float frameEnergyTH = 0, ab_exposure = 1;                         // :116-117
  bool flaggedForMarginalization = false;                           // :119
  std::vector<PointHessian*> pointHessians;                         // :121
  std::vector<PointHessian*> pointHessiansMarginalized, pointHessiansOut;   // :122-123
  std::vector<ImmaturePoint*> immaturePoints;                       // :125
  SE3 worldToCam_evalPT;                                            // :132
  Vec10 state_zero, state, step;                                    // :135-138
  Vec10 state_scaled;                                               // :136; written by the fork-live optimize only: aff_g2l() below does not read it
  SE3 PRE_worldToCam, PRE_camToWorld;                               // :149-150
  std::vector<FrameFramePrecalc> targetPrecalc;                     // :151
  const SE3& get_worldToCam_evalPT() const { return worldToCam_evalPT; }   // :142
  const Vec10& get_state_zero() const { return state_zero; }       // :143
  const Vec10& get_state() const { return state; }                 // :144
  // :155.  The reference returns state_scaled[6..7] = (SCALE_A, SCALE_B) * state[6..7], which setState refreshes.  A driver that sets
  // affFromState gets exactly that; the others hand a, b in through `aff` (10 * (a / 10) would not give them back bit for bit).
  AffLight aff_g2l() const { return affFromState ? AffLight{10.0 * state[6], 1000.0 * state[7]} : aff; }
  void setState(const Vec10& s) { state = s; }                      // :161-181 (state_scaled / PRE_worldToCam there too: host math)
  void setEvalPT(const SE3& T, const Vec10& s) { worldToCam_evalPT = T; state = s; state_zero = s; }   // :198-202
  FrameHessian() {}
  FrameHessian(const FrameHessian&) = delete;                       // shell points into the object
  // test:
  FrameShell shellStore;
  AffLight aff; bool affFromState = false;                          // see aff_g2l()
  int slot = -1;                                                    // the pyramid slot the frame was uploaded to
  std::vector<std::vector<float>> store;                            // the pixels dIp points to
};
enum ResState { IN = 0, OOB, OUTLIER };                             // FullSystem/Residuals.h:49
struct PointHessian {
  EFPoint* efPoint = nullptr;                                       // :377
  float color[SDSO_MAX_RES] = {}, weights[SDSO_MAX_RES] = {};       // :380-381
  float u = 0, v = 0, energyTH = 0;                                 // :385, :387
  FrameHessian* host = nullptr;                                     // :388
  bool hasDepthPrior = false;                                       // :389
  float my_type = 0, idepth_scaled = 0, idepth_zero = 0, idepth = 0, step = 0;   // :391-397
  float idepth_hessian = 0, maxRelBaseline = 0;                     // :402-403
  int numGoodResiduals = 0;                                         // :404
  void setIdepth(float x) { idepth = x; idepth_scaled = x; }        // :412-415 (SCALE_IDEPTH = 1)
  void setIdepthZero(float x) { idepth_zero = x; }                  // :420-424
  std::vector<PointFrameResidual*> residuals;                       // :427
  std::pair<PointFrameResidual*, ResState> lastResiduals[2] = {{nullptr, OUTLIER}, {nullptr, OUTLIER}};   // :431
  bool isInlierNew() const { return (int)residuals.size() >= 3 && numGoodResiduals >= 4; }   // :465-469; setting_minGoodActiveResForMarg = 3, setting_minGoodResForMarg = 4 (settings.cpp:82-83)
  int id = -1;                                                      // test: index in the window as first uploaded
};

// ---- FullSystem/Residuals.h
struct PointFrameResidual {
  EFResidual* efResidual = nullptr;                                 // :61
  ResState state_state = IN, state_NewState = IN;                   // :66, :72
  double state_energy = 0, state_NewEnergy = 0, state_NewEnergyWithOutlier = 0;   // :69, :75, :78
  PointHessian* point = nullptr;                                    // :84
  FrameHessian *host = nullptr, *target = nullptr;                  // :85-86
  bool isNew = true;                                                // :92
  Vec2f projectedTo[SDSO_MAX_RES];                                  // :95
  Vec3f centerProjectedTo;                                          // :98
  int id = -1;                                                      // test: index in the window as first uploaded
};

// ---- FullSystem/ImmaturePoint.h (default-constructible on purpose, see the head of this file)
struct ImmaturePoint {
  float color[SDSO_MAX_RES], weights[SDSO_MAX_RES];                 // :64-65
  Mat22f gradH;                                                     // :67
  float energyTH;                                                   // :70
  float u, v, u_stereo, v_stereo;                                   // :71-72
  FrameHessian* host;                                               // :73
  int idxInImmaturePoints;                                          // :74
  float quality, my_type;                                           // :76, :78
  float idepth_min, idepth_max, idepth_min_stereo, idepth_max_stereo, idepth_stereo;   // :80-84
  int lastTraceStatus;                                              // :92 (ImmaturePointStatus, :50-56)
  Vec2f lastTraceUV;                                                // :93
  float lastTracePixelInterval;                                     // :94
  int id;                                                           // test: position in the flattened input
};

// ---- OptimizationBackend/EnergyFunctionalStructs.h (the first members in the order the drivers brace-initialise them)
enum EFPointStatus { PS_GOOD = 0, PS_MARGINALIZE, PS_DROP };        // :97
struct EFResidual {
  PointFrameResidual* data; EFFrame* target;                        // :70, :75
  bool isActiveAndIsGoodNEW = false;                                // :89
  int idxInAll = 0;                                                 // :77
  EFPoint* point = nullptr;                                         // :73
  bool isLinearized = false;                                        // :85
};
struct EFPoint {
  PointHessian* data;                                               // :110
  std::vector<EFResidual*> residualsAll;                            // :127
  int stateFlag = PS_GOOD;                                          // :156
  float HdiF = 0, bdSumF = 0, deltaF = 0;                           // :133, :130, :116
  int idxInPoints = 0;                                              // :120
  EFFrame* host = nullptr;                                          // :123
};
struct EFFrame {
  FrameHessian* data; std::vector<EFPoint*> points; int idx;        // :177, :174, :179
  Vec8 delta, delta_prior;                                          // :171, :170
};

// ---- OptimizationBackend/EnergyFunctional.h.  Ownership as in the reference: objects come from raw new, the member that removes one
// deletes it (removePoint also deletes the PointFrameResiduals, which FullSystem does next to it); the graph's owner frees the rest.
struct EnergyFunctional {
  std::vector<EFFrame*> frames;                                     // :88
  int nPoints = 0, nResiduals = 0;                                  // :89
  MatXX HM, lastHS;                                                 // :91, :95
  std::vector<double> bM, lastbS, lastX;                            // :92, :96-97 (VecX there)
  int resInA = 0, resInL = 0, resInM = 0;                           // :94
  Mat18f* adHTdeltaF = 0;                                           // :127
  Mat88 *adHost = 0, *adTarget = 0; Mat88f *adHostF = 0, *adTargetF = 0;   // :131-135
  float cDeltaF[4] = {0, 0, 0, 0};                                  // :139 (VecCf)
  std::vector<EFPoint*> allPoints;                                  // :147
  EnergyFunctional() {}
  EnergyFunctional(const EnergyFunctional&) = delete;
  ~EnergyFunctional() { delete[] adHost; delete[] adTarget; delete[] adHostF; delete[] adTargetF; delete[] adHTdeltaF; }
  // what the reference's std::vector lists do when an entry leaves: the last entry takes its slot and learns its new index
  template <class T, class SetIdx>
  static void swap_out(std::vector<T*>& list, int idx, SetIdx set_idx) {
    list[idx] = list.back();
    set_idx(list[idx], idx);
    list.pop_back();
  }
  void dropResidual(EFResidual* r) {                                // :72, EnergyFunctional.cpp:524-551
    swap_out(r->point->residualsAll, r->idxInAll, [](EFResidual* moved, int k) { moved->idxInAll = k; });
    r->data->efResidual = nullptr;
    nResiduals--;
    delete r;
  }
  void removePoint(EFPoint* p) {                                    // :74, EnergyFunctional.cpp:755-772: the point's residuals go, then the point leaves its host's list
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
  void dropPointsF() {                                              // :77, EnergyFunctional.cpp:739-752: a slot is looked at again after a removal filled it
    for (EFFrame* f : frames) {
      size_t at = 0;
      while (at < f->points.size()) {
        if (f->points[at]->stateFlag == PS_DROP) removePoint(f->points[at]);
        else at++;
      }
    }
  }
};
