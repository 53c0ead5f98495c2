// Host API of the windowed bundle adjustment (C-ABI entry points sdso_ba_*), one translation unit: the kernels, then the host code.
// The window mirrors an EnergyFunctional (src/OptimizationBackend/EnergyFunctional.h:49-150):
// frames / calibration live on the host in double (ba_host.h), points and residuals live in HBM
// (ba_kernels.h).  Call-surface mapping: see include/sdso_abi.h and INTEGRATION.md.
//
//   ba_layout.h    ctx-free, plain C++: validation + pair sort + work lists of an upload (build_window_layout), plan_window_edit
//   ba_window.hip  BaWindowDev, the ctx's BA state and buffer pool, tables, the upload, keep_projections / release_window
//   ba_launch.hip  BaLaunch / BaBatch, single(), launch_*, the deferred folds, the solverMode rules and the layout of BaDev::sol
//   ba_api.hip     per-window step calls and getters: sdso_ba_linearize ... sdso_ba_get_deltas, get_state / post_state / counts, ba_ref_view
//   ba_marg.hip    sdso_ba_marginalize_points / _frame / _frame_dev, sdso_ba_adopt_prior
//   ba_batch.hip   the batch's lifetime, its sdso_ba_batch_* phase calls, the accumulator blocks comm.hip reduces
//   ba_loop.hip    both Gauss-Newton loops: the resident one (single window and batch) and the host loop of sdso_ba_optimize
//   ba_update.hip  sdso_ba_window_plan / _update / _update_activated / _get_order
//   ba_flag.hip    sdso_ba_flag_points: removeOutliers / flagPointsForRemoval on the resident window (the rule itself: ba_flag.h)
// Forward declarations cross the files only where two of them need each other: free_batch / free_optrun (a window's
// release ends the batch, the batch's end ends its loop) and launch_window_gather (the upload is the builder of an updated window).
#include "ba_kernels.hip"
#include "ba_solve.hip"
#include "ba_opt.hip"
#include "ba_tail.hip"
#include "ba_host.h"
#include "ba_solve_alt.hip"   // (after ba_host.h: the SOLVER_* bits and setting_solverModeDelta)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <limits>
#include <chrono>
#include <atomic>
#include <thread>
#include <string>
#include "imm_layout.h"          // ImmActRec: what sdso_ba_window_update_activated reads of an activation
#include "ba_layout.h"
#include "ba_window.hip"
#include "ba_launch.hip"
#include "ba_api.hip"
#include "ba_marg.hip"
#include "ba_batch.hip"
#include "ba_loop.hip"
#include "ba_update.hip"
#include "ba_flag.hip"
