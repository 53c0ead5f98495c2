// Static stereo on gfx950: ImmaturePoint construction, ImmaturePoint::traceStereo and ImmaturePoint::traceOn for a batch of points in one
// launch, the left-right-left matching chain, point activation, and the device-resident immature points of a ctx (sdso_imm_*).
//
// Reference (paths under /root/reference):
//   src/FullSystem/ImmaturePoint.cpp:33-62    ImmaturePoint::ImmaturePoint (colour patch, weights, gradH)
//   src/FullSystem/ImmaturePoint.cpp:33-88    the two constructors
//   src/FullSystem/ImmaturePoint.cpp:94-451   ImmaturePoint::traceStereo; the sub-pixel Gauss-Newton is
//                                             the DSO-native one (twin in traceOn, :707-769)
//   src/FullSystem/ImmaturePoint.cpp:459-828  ImmaturePoint::traceOn
//   src/FullSystem/FullSystem.cpp:1600-1629   makeNewTraces
//   src/FullSystem/FullSystem.cpp:632-781     traceNewCoarseNonKey, traceNewCoarseKey
//   src/FullSystem/FullSystem.cpp:581-613     stereoMatch's loop (sdso_imm_stereo_match)
//   src/FullSystem/FullSystem.cpp:948-957     activatePointsMT STEP 5
//   src/FullSystem/FullSystem.cpp:837-957     activatePointsMT STEP 2-5 in place (sdso_imm_activate)
//   src/FullSystem/CoarseInitializer.cpp:838-972   setFirstStereo, level 0 (sdso_init_set_first_stereo)
//   src/FullSystem/FullSystem.cpp:1533-1573   initializeFromInitializer STEP 3 (sdso_init_from_initializer)
//
// One translation unit in parts: they share static helpers and __forceinline__ device code (trace_on_point, activate_point), which
// separate objects would duplicate.  Per-point arithmetic keeps the reference's operation order (no FP contraction) => statuses, bestIdx
// and all outputs are bit-identical to the CPU path.
//   trace_dev.h       the epipolar search stated once, TraceDev, the constants, the fresh-point writer, the readable-pattern rule
//   imm_layout.h      ctx-free, plain C++: the members of a resident point, the remove order of STEP 5 and its closed form
//   stereo_trace.hip  the kernels that run the search: k_immature_init, k_trace_stereo_blk (a workgroup per 16 points), trace_on_point /
//                     k_trace_on (a wave per point)
//   stereo_batch.hip  TraceBatch (its members and private areas by name), the ctx's StereoState, sdso_immature_init_batch,
//                     sdso_trace_stereo_* and sdso_trace_on_batch
//   stereo_match.hip  the left-right-left chain: trace_pair_bind, launch_fresh_trace, stereo_match_chain_dev, sdso_stereo_match_batch
//   activate.hip      activate_point, k_activate_points, sdso_activate_points_batch
//   imm_compact.hip   ordered compaction (segcount / scan / segwrite), the block-wide scan, one atomic per wave for a predicate
//   imm_set.hip       the resident set: ImmHost, ImmState, the flat index over named hosts, add / count / get / put / remove / release
//   imm_trace.hip     sdso_imm_trace: traceOn in place and the stereo chain of the non-key trace
//   imm_match.hip     sdso_imm_stereo_match: stereoMatch's loop on a group of the set, its kept results and dense map
//   imm_activate.hip  sdso_imm_activate: activatePointsMT STEP 2-5 on the set
//   init_stereo.hip   sdso_init_*: the live part of CoarseInitializer::setFirstStereo and STEP 3 of initializeFromInitializer
#include "sdso_internal.h"
#include "distmap_dev.h"
#include "trace_dev.h"
#include "imm_layout.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace sdso;

#include "stereo_trace.hip"
#include "stereo_batch.hip"
#include "stereo_match.hip"
#include "activate.hip"
#include "imm_compact.hip"
#include "imm_set.hip"
#include "imm_trace.hip"
#include "imm_match.hip"
#include "imm_activate.hip"
#include "init_stereo.hip"
