// Device side of the windowed BA for gfx950 (descriptor and conventions: ba_kernels.h), in parts.  ba.hip includes this hub, then the
// solver's kernels (ba_solve.hip, ba_opt.hip, ba_tail.hip, ba_solve_alt.hip).  Reference arithmetic (paths under the reference's root):
//   ba_jac.h      the RawResidualJacobian on the device (J_*, jdev, JV, load_J), jac_delta and JAC_TAKE_DATA on a loaded record,
//                 the tiled sampler (interp33_tiled), block_sum_d
//   ba_lin.hip    PointFrameResidual::linearize, every statement once (LIN_*, project_pattern)   src/FullSystem/Residuals.cpp:83-336
//                 linearize_one, the cooperative gather and linearize_coop, k_ba_linearize
//   ba_state.hip  k_ba_apply          PointFrameResidual::applyRes + takeDataF       Residuals.cpp:367-385, EnergyFunctionalStructs.cpp:37-51
//                 k_ba_post_state     linearizeAll_Reductor(true) per residual       src/FullSystem/FullSystemOptimize.cpp:62-78
//                 k_ba_fixlin         EFResidual::fixLinearizationF                  EnergyFunctionalStructs.cpp:96-123
//                 k_ba_reset_flagged, k_ba_unmask, k_ba_init_res, k_ba_reset_all      resetOOB: FullSystem.cpp:1012-1016, FullSystemOptimize.cpp:886-892
//   ba_top.hip    k_ba_accum_top      AccumulatedTopHessianSSE::addPoint<mode>       src/OptimizationBackend/AccumulatedTopHessian.cpp:36-198
//                 k_ba_lin_fused      linearize + applyRes + takeDataF + addPoint<0> in one pass (the hot kernel)
//                 k_ba_lenergy        EnergyFunctional::calcLEnergyPt                EnergyFunctional.cpp:354-417
//                 k_ba_fold_top, k_ba_zero_topL   the chunks' partials -> the packed accumulator
//   ba_sc.hip     k_ba_sc_host        AccumulatedSCHessianSSE::addPoint              AccumulatedSCHessian.cpp:34-103
// The parts are one translation unit: they share force-inlined device code and macros (JV, LIN_PROJECT_FEJ), in this order.
#include "ba_kernels.h"
#include "ba_jac.h"
#include "ba_lin.hip"
#include "ba_state.hip"
#include "ba_top.hip"
#include "ba_sc.hip"
