// FullSystem::removeOutliers + FullSystem::flagPointsForRemoval as ONE decision per point, stated once: k_ba_flag_points (ba_flag.hip)
// evaluates it per lane, csrc/test_ba_flag.cpp checks it on a CPU.  Plain C++, no HIP type besides the __host__ __device__ marks.
//
// Reference:
//   src/FullSystem/FullSystemOptimize.cpp:1063-1084  removeOutliers: residuals.size() == 0 -> PS_DROP
//   src/FullSystem/FullSystem.cpp:965-1056           flagPointsForRemoval
//   src/FullSystem/HessianBlocks.h:439-469           PointHessian::isOOB / isInlierNew
//   src/FullSystem/FullSystemOptimize.cpp:165-195    linearizeAll(true): lastResiduals[k].second takes state_state (:167-173) BEFORE the
//                                                    residuals on toRemove lose .first and leave ph->residuals (:176-195)
// The point's residuals are fed one by one in any order (flag_point_add: nothing below depends on the order), then flag_point_decide.
// Not here: the re-linearisation and fixLinearizationF of FullSystem.cpp:1012-1021 (sdso_ba_marginalize_points does them; they change
// no value the decision reads), and the toKeep list of :974-976, which is dead (its loop condition never holds).
#pragma once
#include "../../include/sdso_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_FLAG_HD __host__ __device__ __forceinline__
#else
#define BA_FLAG_HD inline
#endif

namespace sdso {

// ResState (src/FullSystem/Residuals.h:49)
constexpr int FLAG_RS_IN = 0, FLAG_RS_OOB = 1, FLAG_RS_OUTLIER = 2;
constexpr int FLAG_NONE = 255;   // "no such residual" / "no caller value"

struct FlagSettings {
  int minGoodActiveResForMarg;   // settings.cpp:82  3
  int minGoodResForMarg;         // settings.cpp:83  4
  float minIdepthH_marg;         // settings.cpp:57  50
};

// what the walk over one point's residuals leaves
struct FlagPointAcc {
  int n = 0;                     // ph->residuals.size() after the closing linearizeAll(true): the residuals not on toRemove
  int visInToMarg = 0;           // HessianBlocks.h:442-448
  int last[2] = {FLAG_NONE, FLAG_NONE};   // state_state of the residual into frame nf-1-k, on toRemove or not (FullSystemOptimize.cpp:167-173)
};

// one residual of the point: its target frame, its state_state and whether linearizeAll(true) put it on toRemove
BA_FLAG_HD void flag_point_add(FlagPointAcc& a, int target, int state, bool removed, int nf, unsigned frame_marg_mask) {
  if (target == nf - 1) a.last[0] = state;
  if (target == nf - 2) a.last[1] = state;
  if (removed) return;                                     // :184-195: no longer in ph->residuals
  a.n++;
  if (state == FLAG_RS_IN && ((frame_marg_mask >> target) & 1u)) a.visInToMarg++;   // HessianBlocks.h:445-447
}

// lastResiduals[k].second: the caller's value where it gives one (the history of a residual an earlier keyframe dropped), else the
// window's, else what optimizeImmaturePoint initialised it with (FullSystemOptPoint.cpp:204-207: ResState::OOB)
BA_FLAG_HD int flag_point_last(int derived, int gone) {
  if (gone != FLAG_NONE) return gone;
  return derived != FLAG_NONE ? derived : FLAG_RS_OOB;
}

// PointHessian::isOOB (HessianBlocks.h:439-462): 0 = false, else the number of the clause that returned true
BA_FLAG_HD int flag_point_is_oob(int n, int visInToMarg, int numGoodResiduals, int last0, int last1, const FlagSettings& S) {
  if (n >= S.minGoodActiveResForMarg && numGoodResiduals > S.minGoodResForMarg + 10 && n - visInToMarg < S.minGoodActiveResForMarg) return 1;   // :449-452
  if (last0 == FLAG_RS_OOB) return 2;                                           // :458
  if (n < 2) return 0;                                                          // :459
  if (last0 == FLAG_RS_OUTLIER && last1 == FLAG_RS_OUTLIER) return 3;           // :460
  return 0;
}

// PointHessian::isInlierNew (HessianBlocks.h:465-469)
BA_FLAG_HD bool flag_point_is_inlier_new(int n, int numGoodResiduals, const FlagSettings& S) {
  return n >= S.minGoodActiveResForMarg && numGoodResiduals >= S.minGoodResForMarg;
}

// The decision (SDSO_PT_*).  last0 / last1: flag_point_last of the two slots; host_marg: the host frame is flaggedForMarginalization.
// oob_clause (may be null): what flag_point_is_oob returned, 0 where the decision fell before it
BA_FLAG_HD int flag_point_decide(int n, int visInToMarg, int last0, int last1, float idepth, int numGoodResiduals, float idepth_hessian, bool host_marg,
                                 const FlagSettings& S, int* oob_clause = nullptr) {
  if (oob_clause) *oob_clause = 0;
  if (n == 0) return SDSO_PT_DROP_NO_RESIDUAL;             // FullSystemOptimize.cpp:1073 (FullSystem.cpp:997's second operand never fires after it)
  if (idepth < 0) return SDSO_PT_DROP_NEGATIVE;            // FullSystem.cpp:997 (idepth_scaled = SCALE_IDEPTH * idepth, SCALE_IDEPTH = 1)
  const int oob = flag_point_is_oob(n, visInToMarg, numGoodResiduals, last0, last1, S);
  if (oob_clause) *oob_clause = oob;
  if (oob || host_marg) {                                  // :1004
    if (flag_point_is_inlier_new(n, numGoodResiduals, S))  // :1008
      return idepth_hessian > S.minIdepthH_marg ? SDSO_PT_MARGINALIZE : SDSO_PT_DROP_WEAK;   // :1026-1034
    return SDSO_PT_DROP_NOT_INLIER;                        // :1037-1040
  }
  return SDSO_PT_KEEP;
}

}  // namespace sdso
