// sdso_shim.h — header-only C++ host layer that keeps the reference's call surface
// (CoarseTracker / EnergyFunctional / ImmaturePoint) on top of the C-ABI of
// libsdso_hip.so.  It is written against the reference's member NAMES through templates, so the same
// header compiles
//   * inside the reference tree against its real types (Eigen/Sophus: SE3 = Sophus::SE3d, AffLight,
//     FrameHessian, CalibHessian, EnergyFunctional, EFFrame/EFPoint/EFResidual, ImmaturePoint), and
//   * in this repository against the small stand-ins of host/test_shim.cpp (Eigen is not available here).
// Nothing here computes on the CPU what the library computes on the GPU; the shim only marshals.
//
// Reference signatures mirrored (paths under /root/reference/src):
//   bool CoarseTracker::trackNewestCoarse(FrameHessian*, SE3&, AffLight&, int coarsestLvl, Vec5 minResForAbort, ...)   FullSystem/CoarseTracker.h:62-66
//   void CoarseTracker::makeK(CalibHessian*)                                                                        FullSystem/CoarseTracker.h:76
//   Vec6 CoarseTracker::calcRes(int lvl, SE3 refToNew, AffLight aff_g2l, float cutoffTH) + calcGSSSE(lvl,H,b,...)    FullSystem/CoarseTracker.cpp:600, :537
//   void EnergyFunctional::solveSystemF(int iteration, double lambda, CalibHessian*)                                 OptimizationBackend/EnergyFunctional.h:74
//   void EnergyFunctional::marginalizePointsF()                                                                      OptimizationBackend/EnergyFunctional.h:69
//   float FullSystem::optimize(int mnumOptIts)                                                                       FullSystem/FullSystemOptimize.cpp:871
//   ImmaturePointStatus ImmaturePoint::traceStereo(FrameHessian* frame, Mat33f K, bool mode_right)                   FullSystem/ImmaturePoint.h:89
//   void CoarseTracker::setCoarseTrackingRef(std::vector<FrameHessian*>, FrameHessian* fh_right, CalibHessian)        FullSystem/CoarseTracker.h:71-72
//   void CoarseTracker::setCTRefForFirstFrame(std::vector<FrameHessian*>)                                           FullSystem/CoarseTracker.cpp:794-805
//   void CoarseTracker::debugPlotIDepthMap(float* minID, float* maxID, std::vector<IOWrap::Output3DWrapper*>& wraps)    FullSystem/CoarseTracker.h:94, CoarseTracker.cpp:1071-1176
//   void CoarseTracker::debugPlotIDepthMapFloat(std::vector<IOWrap::Output3DWrapper*>& wraps)                         FullSystem/CoarseTracker.h:95, CoarseTracker.cpp:1178-1188
//   double PointFrameResidual::linearize(CalibHessian*) / void applyRes(bool)                                        FullSystem/Residuals.h:103, :113
//   AccumulatedTopHessianSSE::{setZero, addPoint<mode>, addPointsInternal<mode>, stitchDouble, stitchDoubleMT}        OptimizationBackend/AccumulatedTopHessian.h:66-97, :162-169
//   AccumulatedSCHessianSSE::{setZero, addPoint, addPointsInternal, stitchDouble, stitchDoubleMT}                     OptimizationBackend/AccumulatedSCHessian.h:66-96, :155-160
//   EnergyFunctional::{calcLEnergyF_MT, calcMEnergyF, setDeltaF, setAdjointsF}                                       OptimizationBackend/EnergyFunctional.h:75-86
//   CoarseDistanceMap::{makeK, makeDistanceMap, addIntoDistFinal, fwdWarpedIDDistFinal, K, Ki}                          FullSystem/CoarseTracker.h:165-197
//   void FullSystem::activatePointsMT() STEP 1-2                                                                      FullSystem/FullSystem.cpp:796-902
//   the tail of optimizeImmaturePoint + STEP 4 of activatePointsMT into the resident window (WindowedBA::updateActivated)   FullSystem/FullSystemOptPoint.cpp:196-237, FullSystem.cpp:919-945
//   void FullSystem::makeNewTraces(FrameHessian*, FrameHessian*, float*), traceNewCoarseNonKey / traceNewCoarseKey(fh, fh_right)    FullSystem/FullSystem.cpp:1600, :632, :745
//   the loop of void FullSystem::stereoMatch(ImageAndExposure*, ImageAndExposure*, int, cv::Mat&)                      FullSystem/FullSystem.cpp:579-613
//   Undistort::{undistort<T>, getK, getSize, getOriginalSize, getBl, isValid, loadPhotometricCalibration}               util/Undistort.h:63-104
//   void KeyFrameDisplay::setFromKF(FrameHessian* fh, CalibHessian* HCalib)                                          IOWrapper/Pangolin/KeyFrameDisplay.h:62, .cpp:85-165
//   bool KeyFrameDisplay::refreshPC(bool canRefresh, float scaledTH, float absTH, int mode, float minBS, int sparsity)  IOWrapper/Pangolin/KeyFrameDisplay.h:66, .cpp:174-323
//   void CoarseInitializer::setFirstStereo(CalibHessian*, FrameHessian* newFrameHessian, FrameHessian* newFrameHessian_Right)   FullSystem/CoarseInitializer.h:108, .cpp:838-1034
//   STEP 3 of void FullSystem::initializeFromInitializer(FrameHessian* newFrame)                                  FullSystem/FullSystem.cpp:1533-1573
//   the swap of coarseTracker / coarseTracker_forNewKF (CoarseTracker::exportRef / adoptRef) and the frames deliverTrackedFrame queues (Device::exportFrame / importFrame)   FullSystem/FullSystem.cpp:1102-1109, :1203-1221
//   float FullSystem::optimize(int mnumOptIts), the body the fork compiles (g2o LM over EdgeLBASE3PosePhotoIdepthCamDSO)      FullSystem/FullSystemOptimize.cpp:402-868
#pragma once
#include "shim/device.h"        // Error, Shared, Device.  (One part per concern; this header is the whole layer, namespace sdso_shim.)
#include "shim/marshal.h"       // the marshalling rules the parts share, each stated once
#include "shim/tracker.h"       // CoarseTracker
#include "shim/windowed_ba.h"   // WindowedBA, and in detail its bodies that touch only the pointer graph or plain buffers
#include "shim/accumulators.h"  // AccumulatedTopHessianSSE, AccumulatedSCHessianSSE
#include "shim/immature.h"      // traceStereoAll, traceStereo, traceOnAll, traceOn, ImmaturePoints
#include "shim/activation.h"    // CoarseDistanceMap, updateMinActDist, selectPointsToActivate
#include "shim/selector.h"      // PixelSelector, marginalizeFrame
#include "shim/init.h"          // CoarseInitializer
#include "shim/undistort.h"     // Undistort
#include "shim/map.h"           // PointMap, KeyFrameDisplay
#include "fork_live.h"          // optimizeForkLive: the fork-live FullSystem::optimize (beside the parts, see its head)
