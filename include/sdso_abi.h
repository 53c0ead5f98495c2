/*
 * sdso_abi.h — C-ABI of libsdso_hip.so, the MI355X (gfx950) implementation of Stereo-DSO's
 * photometric direct-alignment hot path.
 *
 * The reference (gyubeomim/stereo-dso-g2o) has no FFI layer: the path sits behind plain C++
 * member functions called by FullSystem.  Each entry point below names the reference member
 * function (file:line under /root/reference) whose work it performs; the header-only C++ shims
 * in stereo-dso-g2o_amd/host/ keep the reference's class/method names on top of these calls
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - every function returns 0 (SDSO_OK) or a negative SDSO_ERR_* code; nothing throws;
 *     sdso_last_error() returns a static/ctx-owned message for the last failure on that ctx.
 *   - all pointers are caller-owned HOST buffers unless the name ends in _dev (device pointer).
 *   - matrices are row-major unless stated; SE3 = 3x3 rotation (row-major) + translation.
 *   - one ctx = one GPU + one HIP stream; calls on one ctx must come from one thread at a time
 *     (the reference serialises the same objects under trackMutex / mapMutex,
 *     src/FullSystem/FullSystem.cpp:1063, :1345).
 *   - there is NO CPU fallback: without a usable HIP device sdso_ctx_create fails with
 *     SDSO_ERR_NODEV and every other call fails with SDSO_ERR_STATE.
 */
#ifndef SDSO_ABI_H
#define SDSO_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDSO_OK 0
#define SDSO_ERR_ARG (-1)
#define SDSO_ERR_HIP (-2)
#define SDSO_ERR_NODEV (-3)
#define SDSO_ERR_STATE (-4)

#define SDSO_PYR_LEVELS 6      /* src/util/settings.h:46  PYR_LEVELS */
#define SDSO_PATTERN 8         /* src/util/settings.h:177 patternNum */
#define SDSO_MAX_RES 8         /* src/util/NumType.h:37  MAX_RES_PER_POINT */
#define SDSO_CPARS 4           /* src/util/NumType.h:47  CPARS */
#define SDSO_J_FLOATS 74       /* RawResidualJacobian payload, src/OptimizationBackend/RawResidualJacobian.h:32-65 */
#define SDSO_TOP_FLOATS 91     /* AccumulatorApprox packed sums 55+30+6, MatrixAccumulators.h:595-614 */

typedef struct sdso_ctx sdso_ctx;

/* ------------------------------------------------------------------ context */
int sdso_ctx_create(int device_ordinal, sdso_ctx** out);
void sdso_ctx_destroy(sdso_ctx* ctx);
const char* sdso_last_error(const sdso_ctx* ctx);
/* the HIP stream (hipStream_t) all kernels of this ctx are launched on */
void* sdso_ctx_stream(sdso_ctx* ctx);
int sdso_ctx_sync(sdso_ctx* ctx);
/* Split the device's CUs between two streams of the ctx (hipExtStreamCreateWithCUMask): aux_cus of them for the Schur accumulation and the
 * fused tail kernel of a batch's GN iteration (sdso_ba_batch_schur / sdso_ba_batch_solve_step), the rest for everything else — so that the
 * tail of one ctx's batch owns its CUs while another ctx's linearisation streams on the others.  stride 0: the lowest CU indices; stride s:
 * an equal share out of every s indices.  aux_cus 0 removes the partition.  Streams are re-created: call before sdso_ctx_stream is used.
 * No counterpart in the reference (a schedule); results are bit-identical with and without it. */
int sdso_ctx_partition_cus(sdso_ctx* ctx, int aux_cus, int stride);

/* Optional kernel timing with HIP events recorded on the ctx stream around launches.  on = 1: the dominant kernel of each workload
 * ("k_track_eval", "k_track_lm", "k_ba_lin_fused", "k_ba_linearize", "k_trace_stereo", "k_ingest_level0", ...); on = 2: also the secondary ones
 * ("k_ba_sc", "k_ba_tail", "k_ba_accum_top") — every bracket costs two event records on the stream, which a timed loop should only
 * pay for the kernel it reports; on = 0: off.
 * sdso_prof_read synchronises the stream and returns the accumulated milliseconds / launch count. */
int sdso_prof_enable(sdso_ctx* ctx, int on);
int sdso_prof_reset(sdso_ctx* ctx);
int sdso_prof_read(sdso_ctx* ctx, const char* kernel, double* total_ms, long* launches);

/* Self-test of the device's Lie-group arithmetic (the SE3::exp / product / inverse that the resident tracker LM and GN loops run in
 * kernels): for n tangents xi (6n; translation first, rotation last, se3.hpp:395-397) T_exp[i] = exp(xi_i), T_inv[i] = exp(xi_i)^-1,
 * T_mul_next[i] = exp(xi_i) * exp(xi_(i+1 mod n)), each as R (9, row-major) then t (3).  tests/test_oracle_se3.py puts the Sophus
 * fixtures of thirdparty/Sophus/sophus/test_se3.cpp:40-82 through it. */
int sdso_selftest_se3(sdso_ctx* ctx, int n, const double* xi, double* T_exp, double* T_inv, double* T_mul_next);

/* ------------------------------------------------------------------ pyramids
 * FrameHessian::dIp[lvl] (src/FullSystem/HessianBlocks.h:107-108): Vector3f {I, dx, dy} per pixel.
 * Images are immutable after FrameHessian::makeImages (HessianBlocks.cpp:141-203), so they are
 * mirrored once into device memory and addressed by an integer slot. */
int sdso_pyramid_levels(int w, int h); /* src/util/globalCalib.cpp:52-58 */
int sdso_upload_pyramid(sdso_ctx* ctx, int frame_slot, int levels, const int* w, const int* h,
                        const float* const* dIp /* [levels] AoS float3, w*h*3 floats each */);
/* FrameHessian::makeImages on the device from the level-0 irradiance image (w*h floats). */
int sdso_make_pyramid(sdso_ctx* ctx, int frame_slot, int w, int h, const float* color);
/* Photometric calibration for the pixel selection (setting_gammaWeightsPixelSelect == 1): absSquaredGrad of every pyramid built or
 * uploaded after the call is multiplied by CalibHessian::getBGradOnly(I)^2 (HessianBlocks.cpp:194-198, HessianBlocks.h:356-362).
 * B = CalibHessian::B (256 floats); NULL = identity response (weight exactly 1, the default).
 * sdso_gamma_from_binv = FullSystem::setGammaFunction (FullSystem.cpp:210-234): B from the inverse response table. */
int sdso_set_gamma(sdso_ctx* ctx, const float* B /* 256 or NULL */);
int sdso_gamma_from_binv(const float* BInv /* 256 */, float* B /* 256 */);
/* copy level `lvl` back as AoS float3 (tests) */
int sdso_download_pyramid_level(sdso_ctx* ctx, int frame_slot, int lvl, float* dI_out);
/* FrameHessian::absSquaredGrad[lvl] (HessianBlocks.h:109) as the device holds it: w_l*h_l floats */
int sdso_download_abs_grad(sdso_ctx* ctx, int frame_slot, int lvl, float* out);
int sdso_release_pyramid(sdso_ctx* ctx, int frame_slot);

/* ------------------------------------------------------------------ frame ingest
 * Undistort::undistort<T> (src/util/Undistort.cpp:398-489, called from DatasetReader.h:222) followed by FrameHessian::makeImages
 * (HessianBlocks.cpp:141-203): raw 8- or 16-bit camera images go in, device pyramids come out, with the bits of the reference's
 * undistort followed by sdso_make_pyramid.  Reading calibration and image files (readFromFile's sscanfs, ImageRW) stays with the caller.
 * Not built: the benchmark-only geometric noise (benchmark_varNoise, :416-451), applyBlurNoise (:494-583) — both zero by default
 * (settings.cpp:126-127) — and PhotometricUndistorter::unMapFloatImage (:195-219).
 *
 * sdso_undistort_make_remap — host only, no ctx — is the part of Undistort::readFromFile behind the parsing (:793-949) for callers that
 * have no Undistort object:
 *   model      : which distortCoordinates body runs (:974-1236), in the reference's float / double promotion
 *   parsOrg    : 5 doubles (Pinhole, FOV) or 8 (RadTan, Equidistant, KannalaBrandt), in pixels; when parsOrg[2] < 1 && parsOrg[3] < 1 the
 *                "relative format" rescale of :793-809 is applied first
 *   out_mode   : SDSO_RECTIFY_CROP = makeOptimalK_crop (:586-709; SDSO_ERR_ARG where the reference exits after 500 shrink steps);
 *                SDSO_RECTIFY_NONE (:882-895) needs w == wOrg && h == hOrg and sets *passthrough; SDSO_RECTIFY_EXPLICIT takes
 *                out_calib = relative fx fy cx cy (:896-909); SDSO_RECTIFY_FULL is assert(false) in the reference (:711-714): SDSO_ERR_ARG
 *   K          : the rectified fx fy cx cy (Undistort::getK)
 *   remapX/Y   : w*h floats each as the loop of :919-949 leaves them, -1 where the source lies outside — its quirks included: :937 assigns
 *                ix in the iy == hOrg-1 case and :939 tests iy < wOrg-1 */
#define SDSO_CAM_PINHOLE 0
#define SDSO_CAM_FOV 1
#define SDSO_CAM_RADTAN 2
#define SDSO_CAM_EQUIDISTANT 3
#define SDSO_CAM_KANNALABRANDT 4
#define SDSO_RECTIFY_CROP 0
#define SDSO_RECTIFY_NONE 1
#define SDSO_RECTIFY_FULL 2
#define SDSO_RECTIFY_EXPLICIT 3
int sdso_undistort_make_remap(int model, const double* parsOrg, int wOrg, int hOrg, int w, int h, int out_mode,
                              const float* out_calib /* 4, SDSO_RECTIFY_EXPLICIT only */, double* K /* 4 */,
                              float* remapX /* w*h */, float* remapY /* w*h */, int* passthrough);
/* One camera's undistortion tables, uploaded once and resident under the caller-chosen id `calib` (an id in use is replaced once the new
 * tables are complete; if the call fails the id keeps its old ones).  w x h must give pyramid levels of at least 8 pixels each way:
 *   remapX/Y        : Undistort::remapX / remapY (w*h each) — the reference's own arrays or sdso_undistort_make_remap's; NULL = passthrough
 *                     (:481-483; needs w == wOrg && h == hOrg).  A negative remapX yields 0 (:454-456).  An entry that passed :939 but whose
 *                     four taps (int)x, (int)y, +1, +1 do not all lie inside wOrg x hOrg is an out-of-bounds read in the reference; like
 *                     the unrepresentable projections of sdso_distmap_make it counts as outside the image and yields 0.
 *   pixel_bytes     : 1 (MinimalImageB) or 2 (MinimalImage<unsigned short>)
 *   G               : PhotometricUndistorter::G after the normalisation of :114-123, 256 floats for 1-byte pixels, 65536 for 2-byte
 *                     ones; NULL = the reference's !valid
 *   vignetteMapInv  : wOrg*hOrg floats (:179-181) or NULL; required with G in mode 2
 *   photometricCalibration, useExposure : setting_photometricCalibration (settings.cpp:88) 0, 1 or 2 and setting_useExposure (:89) */
int sdso_ingest_calib_create(sdso_ctx* ctx, int calib, int wOrg, int hOrg, int w, int h, const float* remapX, const float* remapY,
                             int pixel_bytes, const float* G, const float* vignetteMapInv, int photometricCalibration, int useExposure);
int sdso_ingest_calib_release(sdso_ctx* ctx, int calib);
/* Undistort::undistort<T>(raw[i], exposure[i], timestamp, factor) steps 1 and 2 and makeImages into pyramid slot frame_slots[i], for the
 * n_images (1 or 2: left and right) images of one frame.  Step 1 is PhotometricUndistorter::processFrame (:222-260): factor * raw when G is
 * NULL, exposure[i] <= 0 or the mode is 0, else G[raw], times vignetteMapInv in mode 2; exposure_out[i] (may be NULL) is exposure[i], or 1
 * with useExposure off (:258-259).  The gamma weighting of sdso_set_gamma applies as for any pyramid built after it.
 * The call only ENQUEUES, like sdso_ba_upload_window: the raw bytes are copied into pinned staging before it returns (the caller's
 * buffers may go away), everything is issued on the ctx stream and nothing synchronises — with one exception: a slot that holds a
 * pyramid of another shape is released and allocated anew, as sdso_make_pyramid does, and that release synchronises the stream (a slot
 * of the calibration's shape, or an empty one, does not).  An unknown calib, a NULL image, a slot named twice or n_images outside 1..2
 * return SDSO_ERR_ARG before any device work and before any slot or staging buffer is touched; a w x h whose pyramid would hold a level
 * below 8 pixels is refused by sdso_ingest_calib_create already, so no slot's shape can fail here. */
int sdso_ingest_frame(sdso_ctx* ctx, int calib, int n_images, const int* frame_slots, const void* const* raw, const float* exposure,
                      float factor, float* exposure_out);

/* ------------------------------------------------------------------ coarse tracker
 * CoarseTracker::calcRes + calcGSSSE (src/FullSystem/CoarseTracker.cpp:600-792, :537-596),
 * DSO-native arithmetic (the residual/Huber/buffer code kept as comments at :699-775). */
typedef struct {
  int lvl;
  int w, h;              /* w[lvl], h[lvl]                       CoarseTracker.cpp:609-610 */
  float fx, fy, cx, cy;  /* fx[lvl]..cy[lvl]                     CoarseTracker.cpp:612-615 */
  float Ki[9];           /* Ki[lvl] = K[lvl].inverse()           CoarseTracker.cpp:130     */
  float RKi[9];          /* R.cast<float>() * Ki[lvl]            CoarseTracker.cpp:617     */
  float t[3];            /* refToNew.translation().cast<float>() CoarseTracker.cpp:618     */
  float affLL[2];        /* AffLight::fromToVecExposure(...).cast<float>()  :621           */
  float ref_b0;          /* lastRef_aff_g2l.b                    CoarseTracker.cpp:542     */
  float cutoffTH;        /* setting_coarseCutoffTH*levelCutoffRepeat        :894           */
  float huberTH;         /* setting_huberTH                      settings.cpp:95           */
} sdso_track_eval_t;

/* pc_u/pc_v/pc_idepth/pc_color[lvl], pc_n[lvl] (CoarseTracker.h:132-140) */
int sdso_track_set_ref(sdso_ctx* ctx, int ref_slot, int lvl, int n, const float* pc_u,
                       const float* pc_v, const float* pc_idepth, const float* pc_color);
int sdso_track_release_ref(sdso_ctx* ctx, int ref_slot);

/* CoarseTracker::makeCoarseDepthL0 (CoarseTracker.cpp:352-534) on the device: STEP1 splat of n weighted inverse depths at
 * integer pixels (u,v) of the newest keyframe `frame_slot` (= lastRef), STEP2 2x2 pyramid sums, STEP3/4 dilation, STEP5
 * normalisation + compaction in raster order, for every level of that pyramid.  The result is installed as tracking
 * reference `ref_slot` exactly as sdso_track_set_ref would; pc_n_out[levels] receives pc_n[lvl].
 * (new_idepth / weight are what STEP1 computes per active point: the stereo-refined idepth — sdso_stereo_match_batch —
 * and sqrtf(1e-3 / (HdiF + 1e-12)), :350.) */
int sdso_track_make_ref(sdso_ctx* ctx, int ref_slot, int frame_slot, int n, const int* u, const int* v,
                        const float* new_idepth, const float* weight, int* pc_n_out);
/* CoarseTracker::setCoarseTrackingRef -> makeCoarseDepthL0 (CoarseTracker.cpp:275-534, 807-826) from the device-resident window `win`
 * after sdso_ba_optimize: STEP1's gather, the L->R->L stereo re-observation, the accept rule and the weight, then STEP2-5, without any
 * per-point data crossing the bus.  lastRef = the window's last frame (its frame_slot), K = the window's current calibration
 * (Hcalib.fxl() .. cyl() after the optimize).
 *   selection : a point is splatted iff its residual into the newest keyframe is in activeResiduals, active and IN after the closing
 *               linearizeAll(true) — lastResiduals[0].first != 0 && lastResiduals[0].second == ResState::IN (:295)
 *   per point : centerProjectedTo as sdso_ba_get_post_state returns it; u = int(cpt[0] + 0.5f), v likewise; both traces take the
 *               interval [0.1f, 1.9f] * cpt[2]; the accept rule of :329-341; weight = sqrtf(1e-3 / (HdiF + 1e-12))
 *   order     : the splat adds the points of one pixel in the order of point_order (window point indices) restricted to the selected
 *               points — pass FrameHessian::pointHessians order, frame by frame, which differs from the window's order once points
 *               have been removed (EnergyFunctional.cpp:755-771 swaps, FullSystem.cpp:1047-1053 compacts).  NULL: window order.
 *   border    : a selected point whose rounded pixel lies outside [2, w-3) x [2, h-3) takes no stereo (new_idepth = cpt[2]); one
 *               outside the image is not splatted.  Both are counted in n_border_out.  The reference reads / writes outside its
 *               arrays there, and sdso_stereo_match_batch refuses such a point; an IN residual has its pattern inside (1.1, w-3), so
 *               the count is expected to be 0.
 *   refusals  : decided before any device work.  SDSO_ERR_STATE: the window has no valid post-state (no optimize call has ended on it,
 *               or sdso_ba_window_update has edited it since), is inside a batch, or holds a linearised residual.  SDSO_ERR_ARG: an
 *               unknown window or frame slot, a right pyramid of another size, a point_order entry out of range or named twice.
 *   sync      : the call reads the number of selected points back once (the launches of the stereo chain and of the splat are sized
 *               by it) and otherwise only enqueues: the templates are allocated for the most points STEP5 can keep, and pc_n reaches
 *               the host behind an event that the next reader of the reference (sdso_track_newest_coarse, sdso_track_get_ref, ...)
 *               waits for.  Asking for pc_n_out waits for that event in the call.  A template that has to grow is allocated anew,
 *               which synchronises once.  sdso_trace_set_gn_mode applies as in sdso_stereo_match_batch.
 * The reference is installed exactly as by sdso_track_make_ref; n_points_out = the selected points, pc_n_out[levels]; each may be NULL. */
int sdso_track_make_ref_from_window(sdso_ctx* ctx, int ref_slot, int win, int right_slot, float baseline,
                                    const int* point_order /* n_order window point indices, or NULL: window order */, int n_order,
                                    int* n_points_out, int* n_border_out, int* pc_n_out /* levels; each may be NULL */);
/* tests / debugging: STEP1's per-point results of the latest call on ref_slot, in splat order; arrays may be NULL */
int sdso_track_get_ref_points(sdso_ctx* ctx, int ref_slot, int* n, int* point /* window index */, int* u, int* v,
                              float* centerProjectedTo2, uint8_t* status_fwd, uint8_t* status_back, float* new_idepth, float* weight);
/* read a template level back (tests); n_out = pc_n[lvl]; arrays may be NULL */
int sdso_track_get_ref(sdso_ctx* ctx, int ref_slot, int lvl, int* n_out, float* pc_u, float* pc_v,
                       float* pc_idepth, float* pc_color);

/* The keyframe's published depth images: CoarseTracker::debugPlotIDepthMap / debugPlotIDepthMapFloat (CoarseTracker.cpp:1071-1188, called
 * unconditionally by FullSystem::makeKeyFrame, FullSystem.cpp:1444-1445) from the level-0 map idepth[0] of a template.
 *
 * sdso_track_keep_depth_map: off by default, and nothing changes while it is off.  On: every template sdso_track_make_ref or
 * sdso_track_make_ref_from_window builds from then on keeps a copy of its level-0 map (w*h floats, owned by the reference slot) as STEP5
 * leaves it (:492-533): inside [2,w-2) x [2,h-2) the normalised inverse depth or -1, in the two-pixel border the UN-normalised weighted
 * sums of STEP1 and STEP3 — the reference's sort (:1079-1082) counts those too.  A reference installed by sdso_track_set_ref has no map;
 * sdso_track_release_ref frees it. */
int sdso_track_keep_depth_map(sdso_ctx* ctx, int on);
/* debugPlotIDepthMap (:1071-1176) on the kept map of `ref_slot`; `frame_slot` = the pyramid of the frame the template was built on
 * (lastRef->dIp[0]), whose level-0 size must be the map's.
 *   range      : allID = the pixels with idepth > 0 (:1078-1082); minID_new = allID[(int)(n*0.05)], maxID_new = allID[(int)(n*0.95)],
 *                n = size-1 (:1085-1088), selected exactly without sorting.
 *   smoothing  : :1094-1117 against *minID_pt / *maxID_pt (in/out, both or neither).  Both NULL: the new range is used as it is.
 *   image      : rgb (w*h*3 bytes, or NULL) = the B3 image pushDepthImage receives: background :1122-1126, overlay :1129-1163 with
 *                makeJet3B (globalFuncs.h:362-379) and setPixelCirc (MinimalImage.h:100-112), later sources overwriting earlier ones.
 *                idepth (w*h floats, or NULL) = the kept map, the image pushDepthImageFloat receives (:1178-1188).
 *   counts     : [0] allID.size(), [1] the pixels that drew a circle; may be NULL.
 *   deviations : with no positive pixel the reference indexes an empty vector; here the image is the background alone, counts are 0, 0 and
 *                the two range values are left untouched.  A NaN intensity gives a background byte of 0.
 *   refusals   : before any device work.  SDSO_ERR_STATE: the slot keeps no map.  SDSO_ERR_ARG: an unknown slot, a frame of another
 *                size, exactly one of minID_pt / maxID_pt NULL.
 *   sync       : one enqueue of the whole chain, one copy back (range, counts and the images asked for), one synchronisation. */
int sdso_track_depth_image(sdso_ctx* ctx, int ref_slot, int frame_slot, float* minID_pt, float* maxID_pt,
                           uint8_t* rgb /* w*h*3 or NULL */, float* idepth /* w*h or NULL */, int* counts /* 2, or NULL */);
/* The device images of the latest sdso_track_depth_image on `ref_slot`, valid until the next call on it (SDSO_ERR_STATE before the
 * first).  idepth_dev is the kept map itself: debugPlotIDepthMapFloat wraps idepth[0] without copying (:1183). */
int sdso_track_depth_image_dev(sdso_ctx* ctx, int ref_slot, void** rgb_dev /* uint8_t*, w*h*3 */, void** idepth_dev /* float*, w*h */,
                               int* w, int* h);

/* ------------------------------------------------------------------ hand-off between contexts
 * The reference hands two objects from one mutex domain to the other: the tracked frame (fh, fh_right), built under trackMutex and
 * queued for mappingLoop by deliverTrackedFrame (FullSystem.cpp:1203-1221), and the tracking template, built by makeKeyFrame on
 * coarseTracker_forNewKF and swapped in by the tracking thread (FullSystem.cpp:1102-1109).  Each domain has a ctx of its own (one
 * thread per ctx); the calls below pass the device buffers of a pyramid or a template from one ctx to any number of others ON THE SAME
 * DEVICE without a copy and without a trip through the host.
 *
 * sdso_shared is an opaque handle on one reference to a block of level buffers.  It may be passed between threads; every call below
 * is safe from any thread for DIFFERENT ctxs, and follows the one-thread-per-ctx rule for the ctx it names.
 *   frozen    : from its first export on a block is never written again, by any ctx.  A call that would fill the buffers of a slot
 *               that views such a block in place (sdso_upload_pyramid / sdso_make_pyramid / sdso_ingest_frame of the same size,
 *               sdso_track_set_ref, sdso_track_make_ref*, the first-frame template) gives the slot fresh buffers first and leaves
 *               the block to its other holders; sdso_track_set_ref, which replaces one level, copies the slot's other levels over.
 *               A slot that was never exported from or imported into keeps its buffers and their reuse exactly as before.
 *   lifetime  : the holders of a block are the slots that view it and the handles not yet released.  sdso_release_pyramid,
 *               sdso_track_release_ref, sdso_ctx_destroy, a detaching write and sdso_shared_release each drop one reference; the
 *               memory is freed by whoever drops the last one, after all work that any holder enqueued on the block has completed
 *               (a holder that leaves with work in flight leaves an event behind).  A handle outlives its source slot and its
 *               source ctx.
 *   per ctx   : what a ctx derives from a pyramid (the tiled and planar level-0 copies, the pixel selector's map) or keeps next to a
 *               template (the kept level-0 map, the STEP1 records of sdso_track_make_ref_from_window) is that ctx's own and does not
 *               travel: on an imported template sdso_track_depth_image and sdso_track_get_ref_points return SDSO_ERR_STATE, as on a
 *               template without a kept map / not built from a window.
 *   gamma     : a pyramid carries the absSquaredGrad weighting (sdso_set_gamma) of the ctx that BUILT it, whatever the importer's.
 *   refusals  : SDSO_ERR_ARG before any device work: a null argument, an unknown source slot, a handle of the other kind, a
 *               destination ctx on another device than the block's (peer copies are out of scope: frames are replicated per GPU). */
typedef struct sdso_shared sdso_shared;
/* fh / fh_right as deliverTrackedFrame queues them (FullSystem.cpp:1203-1221).  Runs on the source's thread; *out is one more holder
 * of the slot's buffers.  Enqueues one event on the source's stream behind everything enqueued so far (the pyramid may still be on its
 * way, as after sdso_ingest_frame); no host wait. */
int sdso_pyramid_export(sdso_ctx* src, int frame_slot, sdso_shared** out);
/* mappingLoop taking the frame from unmappedTrackedFrames (FullSystem.cpp:1203-1221).  Runs on the destination's thread: the slot
 * gives up what it held and views the block; the destination's stream waits for the export's event.  No copy; no host wait unless
 * the slot held buffers of its own, which are freed as by sdso_release_pyramid.  One handle may be imported into any number of ctxs
 * and slots, the source ctx under another slot included, also after the source slot or ctx is gone. */
int sdso_pyramid_import(sdso_ctx* dst, int frame_slot, sdso_shared* h);
/* coarseTracker_forNewKF as makeKeyFrame leaves it for the swap of FullSystem.cpp:1102-1109.  As sdso_pyramid_export; waits for the
 * template's counts (pc_n) if they are still on their way, and for nothing else. */
int sdso_track_export_ref(sdso_ctx* src, int ref_slot, sdso_shared** out);
/* the swap of FullSystem.cpp:1102-1109 on the tracking thread's ctx.  As sdso_pyramid_import: the slot views the block's levels with
 * their counts.  (A slot that held a template of its own, or a ctx with sdso_g2o_track_* edge sets, frees those behind a wait.) */
int sdso_track_import_ref(sdso_ctx* dst, int ref_slot, sdso_shared* h);
/* kind: 0 pyramid, 1 template; holders: slots + handles (FullSystem.cpp:1203-1221: the queue's entry counts as one) */
int sdso_shared_info(const sdso_shared* h, int* kind, int* device, int* holders);
/* the handle's reference goes (FullSystem.cpp:1203-1221: the frame leaves the queue); the handle is invalid afterwards */
void sdso_shared_release(sdso_shared* h);
/* tests / debugging of the hand-off (FullSystem.cpp:1203-1221): the device addresses behind a slot (SDSO_PYR_LEVELS entries; kind as
 * above) and whether they are a view of an exported block.  They stay the same across in-place rebuilds of a slot nobody exported. */
int sdso_shared_debug_buffers(sdso_ctx* ctx, int kind, int slot, unsigned long long* addr, int* is_view /* may be NULL */);

/* ------------------------------------------------------------------ device buffer pool
 * The hand-off above makes no copy, but the slots around it free and allocate: an import into slots that were the last holders of the
 * previous frame frees its level buffers behind host waits, the builder's next build into an exported slot allocates fresh ones, and
 * several paths synchronise a stream only so that a hipFree is safe.  A pool takes those calls off the per-frame path: with one
 * attached, the level buffers of pyramids, their tiled / planar level-0 copies and the levels of tracking templates are PARKED when
 * they leave a slot and handed out again to the next slot that asks for their size, of any ctx attached to the pool.
 *   the rule   : a parked buffer carries the events of its earlier uses (the block's export event, the event of every holder that left
 *                with work in flight, or one event the ctx records on its stream); whoever takes it has its stream wait for them (no
 *                host wait), and nothing is passed to hipFree before they completed (sdso_pool_trim, the cap).
 *   sizes      : pyramid levels and their level-0 copies by exact byte size; template levels take the smallest parked template level of
 *                1 .. 2 times what they need, and fresh ones are rounded up to four size classes per power of two.
 *   who waits  : nobody under the cap.  A buffer that does not fit under max_parked_bytes, after every completed parked buffer was
 *                freed, is freed behind a host wait for its events (overflow_waits); the last reference to the pool waits for what is
 *                pending and frees everything.
 *   lifetime   : reference-counted: the caller (until sdso_pool_release), every attached ctx, every block exported by an attached
 *                ctx.  The pool may be released while ctxs and handles still refer to it; a handle released last
 *                (sdso_shared_release, no ctx) parks into its block's own pool.
 *   not pooled : the kept depth map, BA windows, immature sets, the map, staging and scratch.
 *   default    : a ctx has no pool, and every call does exactly what it did before pools existed.
 *   refusals   : SDSO_ERR_ARG before any device work: a null argument, a pool of another device than the ctx's; SDSO_ERR_NODEV for a
 *                device ordinal that does not exist. */
typedef struct sdso_pool sdso_pool;
/* hits / misses: buffers handed out from the parked ones / allocated; frees: buffers the pool passed to hipFree; host_waits: host
 * waits made while parking or handing out (0 under the cap); overflow_waits: parks that did not fit; parked_*: what is parked now */
typedef struct { long long hits, misses, frees, host_waits, overflow_waits; long long parked_buffers, parked_bytes; } sdso_pool_stats_t;
/* an empty pool for the ctxs of one device; *out is the caller's reference.  No device work. */
int sdso_pool_create(int device_ordinal, size_t max_parked_bytes, sdso_pool** out);
/* From now on the ctx's level buffers come from and go to `pool` (NULL: none, as before sdso_ctx_set_pool).  Any time, any number of
 * ctxs per pool; what the ctx holds stays where it is and is parked by byte size when it leaves, whoever allocated it.  Runs on the
 * ctx's thread. */
int sdso_ctx_set_pool(sdso_ctx* ctx, sdso_pool* pool);
/* a snapshot; safe from any thread */
int sdso_pool_stats(const sdso_pool* pool, sdso_pool_stats_t* out);
/* frees parked buffers whose events have completed, oldest first, until at most keep_bytes stay parked; no host wait; any thread */
int sdso_pool_trim(sdso_pool* pool, size_t keep_bytes);
/* the caller's reference goes; the handle is invalid afterwards */
void sdso_pool_release(sdso_pool* pool);

/* Host-only helper (no GPU work): fill the evaluation parameters for (level, pose, affine) the way
 * CoarseTracker::makeK (:108-136) and calcRes (:617-621) derive them; cutoffTH =
 * prm->coarseCutoffTH * levelCutoffRepeat. Declared after sdso_track_params_t below. */

/* One fused evaluation = calcRes followed by calcGSSSE on the buffers it filled.
 *   H[64], b[8]  : H_out / b_out after the scaling at CoarseTracker.cpp:581-595 (double)
 *   res[6]       : Vec6 (double) returned by calcRes (:783-789)
 *   n_warped     : buf_warped_n INCLUDING the zero padding to a multiple of 4 (:763-775)
 *   inlier_mask  : optional, n bytes; 1 where the point was appended to buf_warped_*          */
int sdso_track_calc_res_gs(sdso_ctx* ctx, int ref_slot, int frame_slot,
                           const sdso_track_eval_t* ev, double* H, double* b, double* res,
                           int* n_warped, uint8_t* inlier_mask);

/* The same for `nprob` independent (reference, frame, pose) problems in ONE launch. Outputs are
 * arrays of nprob entries (H: nprob*64, b: nprob*8, res: nprob*6, n_warped: nprob). */
int sdso_track_calc_res_gs_batch(sdso_ctx* ctx, int nprob, const int* ref_slots,
                                 const int* frame_slots, const sdso_track_eval_t* evs, double* H,
                                 double* b, double* res, int* n_warped);
/* Asynchronous form used by the benchmark: enqueue only (no host copy, no sync); results stay in
 * the ctx's device result buffer and are fetched with sdso_track_batch_fetch. */
int sdso_track_batch_prepare(sdso_ctx* ctx, int nprob, const int* ref_slots,
                             const int* frame_slots, const sdso_track_eval_t* evs);
int sdso_track_batch_enqueue(sdso_ctx* ctx);
int sdso_track_batch_fetch(sdso_ctx* ctx, double* H, double* b, double* res, int* n_warped);

typedef struct { double R[9]; double t[3]; } sdso_se3_t;
typedef struct { double a, b; } sdso_aff_t;

typedef struct {
  int levels;                               /* pyrLevelsUsed */
  int w[SDSO_PYR_LEVELS], h[SDSO_PYR_LEVELS];
  float fx[SDSO_PYR_LEVELS], fy[SDSO_PYR_LEVELS], cx[SDSO_PYR_LEVELS], cy[SDSO_PYR_LEVELS]; /* makeK :108-136 */
  float ref_exposure, new_exposure;         /* lastRef->ab_exposure, newFrame->ab_exposure */
  sdso_aff_t ref_aff_g2l;                   /* lastRef_aff_g2l */
  int coarsestLvl;
  double minResForAbort[5];
  float coarseCutoffTH;                     /* setting_coarseCutoffTH = 20 */
  float huberTH;                            /* setting_huberTH = 9 */
  int maxIterations[5];                     /* DSO-native {10,20,50,50,50} (CoarseTracker.cpp:861) */
  double affineOptModeA, affineOptModeB;    /* setting_affineOptModeA/B */
} sdso_track_params_t;

typedef struct {
  int good;                    /* the bool trackNewestCoarse returns */
  double lastResiduals[5];     /* NaN where the level was not reached */
  double lastFlowIndicators[3];
  int iterations[5];           /* LM iterations actually run per level */
  int evaluations;             /* total calcRes evaluations */
  long long point_evals;       /* sum of pc_n[lvl] over all evaluations */
} sdso_track_result_t;

void sdso_track_make_eval(const sdso_track_params_t* prm, int lvl, const sdso_se3_t* refToNew,
                          const sdso_aff_t* aff_g2l, float levelCutoffRepeat, sdso_track_eval_t* ev);

/* CoarseTracker::trackNewestCoarse (CoarseTracker.cpp:827-1069), DSO-native LM (the loop kept as
 * comments at :908-1024).  lastToNew / aff_g2l are in/out exactly like the reference's references. */
int sdso_track_newest_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot,
                             const sdso_track_params_t* prm, sdso_se3_t* lastToNew,
                             sdso_aff_t* aff_g2l, sdso_track_result_t* out);
/* The same for `nhyp` independent (reference, frame, initial pose) hypotheses in lock-step: every round evaluates the pending
 * calcRes+calcGSSSE of all unfinished hypotheses in one launch (FullSystem::trackNewCoarse tries up to 53 initial motions one
 * after the other, FullSystem.cpp:305-441).  Every hypothesis follows exactly the evaluation sequence of the single call.
 * prms / lastToNew / aff_g2l / outs are arrays of nhyp entries (in/out like the single call). */
int sdso_track_newest_coarse_batch(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots,
                                   const sdso_track_params_t* prms, sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l,
                                   sdso_track_result_t* outs);

/* ---- the motion tries of FullSystem::trackNewCoarse (FullSystem.cpp:436-511), with the loop's own rules.
 * The loop calls trackNewestCoarse once per initial motion with the running achievedRes as minResForAbort (:445-449), so a later try
 * sees bounds that earlier tries lowered.  Two facts let the tries run side by side all the same:
 *   - the abort test (CoarseTracker.cpp:1032) runs every time a level ends, also after the first pass of a level that is then repeated
 *     with a doubled cutoff (:1036-1040) and whose second pass overwrites lastResiduals[lvl]: the test can be replayed exactly from the
 *     residual of each of those events — the EVENT TRACE of a try, at most six events (five levels and one repetition);
 *   - the evaluations of a try do not depend on minResForAbort until the test fires, and achievedRes only falls (or goes from NaN to
 *     finite): a try that ran under bounds taken at any EARLIER point of the loop recorded every event the loop's own try would have
 *     produced, up to its abort. */
#define SDSO_TRACK_MAX_EVENTS 6
typedef struct {
  int n;                                        /* events recorded, in order, <= SDSO_TRACK_MAX_EVENTS */
  int lvl[SDSO_TRACK_MAX_EVENTS];               /* the level that ended */
  double res[SDSO_TRACK_MAX_EVENTS];            /* lastResiduals[lvl] as written at that event (CoarseTracker.cpp:1029) */
  double flow[SDSO_TRACK_MAX_EVENTS][3];        /* lastFlowIndicators as written at that event (:1030) */
} sdso_track_trace_t;

/* One try of the loop.  The members marked `in` are what the try produced when it ran (sdso_track_new_coarse fills them;
 * sdso_track_tries_replay reads them); the others are what the loop saw. */
typedef struct {
  /* in: the try as it ran */
  sdso_track_trace_t trace;    /* its events, up to its own end (an abort under the bounds it ran with, or the finest level) */
  int end_good;                /* trackNewestCoarse's verdict if no abort fires (CoarseTracker.cpp:1050-1068) */
  sdso_se3_t end_pose;         /* lastToNew_out / aff_g2l_out if no abort fires (:1044-1045, :1065-1066) */
  sdso_aff_t end_aff;
  /* out: the try as the loop saw it */
  int ran;                     /* 0: the loop had stopped before this try (:499-500); nothing below is set then */
  int good;                    /* trackingIsGood (:445) */
  int abort_lvl;               /* the level the test of CoarseTracker.cpp:1032 fired on under the loop's bounds, -1: none */
  int winner;                  /* 1: the try took over (FullSystem.cpp:475-484) */
  double lastResiduals[5];     /* coarseTracker->lastResiduals after the try: NaN for every level below an abort (CoarseTracker.cpp:855) */
  double lastFlowIndicators[3];
  sdso_se3_t pose;             /* lastF_2_fh_this / aff_g2l_this after the try: the inputs where the try aborted */
  sdso_aff_t aff;
} sdso_track_try_t;

typedef struct {
  int haveOneGood;             /* FullSystem.cpp:437, :483 */
  int winner;                  /* index of the try whose pose was kept, -1: none was good */
  int tryIterations;           /* :438, :451 — the tries the loop ran */
  sdso_se3_t pose;             /* lastF_2_fh (:482; tries[0] when no try was good, :507) */
  sdso_aff_t aff;              /* aff_g2l (:481; aff_last_2_l when no try was good, :506) */
  double flowVecs[3];          /* :480; (100,100,100) cannot remain: a winner sets it, no winner sets (0,0,0) (:505) */
  double achievedRes[5];       /* :436, :487-496; handed out as it is, NaNs included (:511) */
} sdso_track_tries_result_t;

/* Host-only, no ctx: the rules of FullSystem.cpp:436-511 over the `in` members of recs[0..ntries-1], in list order.
 *   - the abort test per event: res > 1.5 * achievedRes[lvl] (false for a NaN bound);
 *   - a new winner: good && std::isfinite((float)res0) && !(res0 >= achievedRes[0]) (:475-477);
 *   - the carry, once a try was good: !std::isfinite((float)achievedRes[i]) || achievedRes[i] > res[i] (:490-491) — a NaN residual of
 *     a level the try did not reach never lowers a bound;
 *   - the stop: haveOneGood && achievedRes[0] < lastCoarseRMSE[0] * reTrackThreshold (:499);
 *   - no good try: flowVecs = 0, aff = aff_last_2_l, pose = tries[0] (:503-508).
 * Fills the `out` members of every record (ran = 0 after the stop), *out, and lastCoarseRMSE = achievedRes (:511).
 * SDSO_ERR_ARG, nothing written: a null argument, ntries outside 1..64, a trace with n outside 0..6 or a level outside 0..4. */
#define SDSO_TRACK_MAX_TRIES 64
int sdso_track_tries_replay(int ntries, const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, sdso_track_try_t* recs,
                            double* lastCoarseRMSE, double reTrackThreshold, sdso_track_tries_result_t* out);

/* FullSystem::trackNewCoarse STEP2-4 (FullSystem.cpp:436-511) on the device, DSO-native LM.
 *   prm              as for sdso_track_newest_coarse; coarsestLvl is the caller's pyrLevelsUsed-1 (:448); minResForAbort is ignored
 *   ntries, tries    lastF_2_fh_tries in list order, 1..SDSO_TRACK_MAX_TRIES (the reference builds up to 53, :305-423)
 *   aff_last_2_l     every try starts from it (:442)
 *   lastCoarseRMSE   in: the stop rule reads [0] (:499); out: achievedRes (:511)
 *   reTrackThreshold setting_reTrackThreshold (settings.cpp:79: 1.5; a float there, widened as the comparison of :499 widens it)
 *   recs             optional, ntries records: every member is written
 * Phase 1 is try 0 alone, exactly the launch of sdso_track_newest_coarse with NaN bounds; the rules follow, and where the loop stops
 * there (nearly every frame) the call returns.  Phase 2 runs tries 1..ntries-1 in ONE launch of the batch (sdso_track_newest_coarse_batch:
 * its grid sizing, its repetition with single workgroups), each under achievedRes as it stands after try 0 — bounds no tighter than
 * the loop's own at any later try — and the rules then walk the event traces in list order with the tightening bounds.  The outcome is
 * the sequential loop's on the device's own numbers.  Tries after the one the loop stops at were run for nothing: they are reported
 * with ran = 0.  No wait between tries or phases exists on the device; the two launches are chained by the host.
 * Refusals (SDSO_ERR_ARG, before any device work, nothing written): a null argument; ntries out of range; an unknown reference or
 * frame slot; a frame without the level the call starts on; a level size other than the uploaded one. */
int sdso_track_new_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries,
                          const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold,
                          sdso_track_tries_result_t* out, sdso_track_try_t* recs);

/* ------------------------------------------------------------------ windowed bundle adjustment
 * One "window" mirrors an EnergyFunctional (src/OptimizationBackend/EnergyFunctional.h:49-150) with
 * its frames / points / residuals flattened in EnergyFunctional::makeIDX order (:998-1018):
 * points in allPoints order, residuals grouped by point in residualsAll order. */
typedef struct {
  int nf, np, nr;
  int w, h;                        /* wG[0], hG[0] */
  double calib_value_scaled[4];    /* CalibHessian::value_scaled  fx fy cx cy   HessianBlocks.h:276-349 */
  double calib_value_zero[4];      /* CalibHessian::value_zero (unscaled)                              */
  /* frames */
  const double* evalPT;            /* nf*12  worldToCam_evalPT: R (9) then t (3)      HessianBlocks.h:132 */
  const double* state;             /* nf*10  FrameHessian::state                      HessianBlocks.h:137 */
  const double* state_zero;        /* nf*10  FrameHessian::state_zero                                     */
  const float* ab_exposure;        /* nf */
  const float* frameEnergyTH;      /* nf */
  const int* frameID;              /* nf     frameID==0 carries the pose prior        HessianBlocks.h:239-265 */
  const int* frame_slot;           /* nf     device pyramid slot of each keyframe (product) */
  const float* const* dI;          /* nf     host level-0 images (oracle only; product ignores) */
  /* points */
  const float* u;                  /* np */
  const float* v;                  /* np */
  const float* idepth;             /* np     PointHessian::idepth (== idepth_scaled, SCALE_IDEPTH=1) */
  const float* idepth_zero;        /* np */
  const float* color;              /* np*8 */
  const float* weights;            /* np*8 */
  const int* host;                 /* np     host frame index (EFFrame::idx) */
  const uint8_t* hasDepthPrior;    /* np */
  /* residuals */
  const int* res_point;            /* nr     non-decreasing */
  const int* res_target;           /* nr */
  const uint8_t* res_state;        /* nr     ResState {IN=0,OOB=1,OUTLIER=2}          Residuals.h:49 */
  /* marginalisation prior and nullspaces */
  const double* HM;                /* (8nf+4)^2 */
  const double* bM;                /* 8nf+4 */
  /* settings */
  int solverMode;                  /* setting_solverMode (settings.h:32-43): every bit solveSystemF reads is honoured (SVD, SVD_CUT7,
                                      ORTHOGONALIZE_SYSTEM, REMOVE_POSEPRIOR, USE_GN, FIX_LAMBDA, ORTHOGONALIZE_X[_LATER]); SVD and
                                      ORTHOGONALIZE_SYSTEM windows are solved per window (not in sdso_ba_batch_*) */
  double affineOptModeA, affineOptModeB;
  int forceAcceptStep;             /* setting_forceAceptStep */
  /* bookkeeping FullSystem::linearizeAll(true) updates at the end of optimize (FullSystemOptimize.cpp:64-77); each may be NULL */
  const float* maxRelBaseline;     /* np     PointHessian::maxRelBaseline   (NULL: 0)                              */
  const int* numGoodResiduals;     /* np     PointHessian::numGoodResiduals (NULL: 0)                              */
  const uint8_t* res_isNew;        /* nr     PointFrameResidual::isNew      (NULL: 1, what Residuals.cpp:79 sets)  */
} sdso_ba_window_t;

int sdso_ba_upload_window(sdso_ctx* ctx, int win, const sdso_ba_window_t* W);
int sdso_ba_release_window(sdso_ctx* ctx, int win);

/* FullSystem::linearizeAll(false) over every residual (FullSystemOptimize.cpp:142-203) =
 * PointFrameResidual::linearize (Residuals.cpp:83-336).  Returns the summed energy (stats[0]). */
int sdso_ba_linearize(sdso_ctx* ctx, int win, double* energy);
/* fetch what the latest linearisation produced (any pointer may be NULL).  After the FUSED linearise + applyRes + accumulate kernel
 * (sdso_ba_batch_accumulate, the resident loop) the records were written straight into EFResidual::J's slot — the swap of
 * takeDataF (EnergyFunctionalStructs.cpp:39) is skipped because the swapped-out copy is dead in the accepted-step flow — and are
 * returned from there, for applied (IN) and not applied (OUTLIER) residuals alike.
 *   J[nr*74] in RawResidualJacobian field order: resF8 Jpdxi0(6) Jpdxi1(6) Jpdc0(4) Jpdc1(4) Jpdd(2)
 *            JIdx0(8) JIdx1(8) JabF0(8) JabF1(8) JIdx2(4) JabJIdx(4) Jab2(4)
 *   newState[nr], newEnergy[nr], newEnergyWithOutlier[nr], projectedTo[nr*16], centerProjectedTo[nr*3] */
int sdso_ba_get_linearization(sdso_ctx* ctx, int win, float* J, uint8_t* newState, float* newEnergy,
                              float* newEnergyWithOutlier, float* projectedTo,
                              float* centerProjectedTo);
/* PointFrameResidual::applyRes(true) for every residual (Residuals.cpp:367-385) incl.
 * EFResidual::takeDataF (EnergyFunctionalStructs.cpp:37-51). */
int sdso_ba_apply_res(sdso_ctx* ctx, int win);
int sdso_ba_get_residual_state(sdso_ctx* ctx, int win, uint8_t* state, uint8_t* isActive,
                               float* JpJdF /* nr*8 */);
/* EFResidual::J (the record takeDataF swapped in, EnergyFunctionalStructs.cpp:39) of every residual, J[nr*74] in the field order of
 * sdso_ba_get_linearization; rows of residuals that are not active are unspecified (the reference never reads them either:
 * AccumulatedTopHessian.cpp:49 / EnergyFunctional.cpp:675 skip !isActive()). */
int sdso_ba_get_ef_jacobians(sdso_ctx* ctx, int win, float* J);

/* accumulateAF_MT + accumulateLF_MT + accumulateSCF_MT up to (not including) the stitch
 * (EnergyFunctional.cpp:212-269; AccumulatedTopHessian.cpp:36-198; AccumulatedSCHessian.cpp:34-103). */
int sdso_ba_accumulate(sdso_ctx* ctx, int win);
/* packed accumulator block of this window, as all-reduced across ranks:
 *   [ topA nf*nf*91 | topL nf*nf*91 | accD nf^3*64 | accE nf*nf*32 | accEB nf*nf*8 | accHcc 16 | accbc 4 | nresA nresL ]
 * sdso_ba_accum_floats gives its length; _dev returns the device pointer (float*) for RCCL. */
int sdso_ba_accum_floats(int nf);
int sdso_ba_accum_dev(sdso_ctx* ctx, int win, void** dev_ptr);
int sdso_ba_get_accumulators(sdso_ctx* ctx, int win, float* packed);
int sdso_ba_set_accumulators(sdso_ctx* ctx, int win, const float* packed); /* after a host-side reduction */
int sdso_ba_get_point_terms(sdso_ctx* ctx, int win, float* HdiF, float* bdSumF, float* Hdd_accAF,
                            float* bd_accAF, float* Hcd_accAF /* np*4 */);

/* stitch (AccumulatedTopHessian.cpp:265-337, AccumulatedSCHessian.cpp:106-195) + the rest of
 * EnergyFunctional::solveSystemF (EnergyFunctional.cpp:838-995) + resubstituteF_MT (:272-341).
 *   x[8nf+4]     : lastX
 *   H,b          : lastHS, lastbS (may be NULL)
 *   frame_step   : nf*8  (FrameHessian::step head<8>), calib_step: 4 */
int sdso_ba_solve(sdso_ctx* ctx, int win, int iteration, double lambda, double* x, double* HS,
                  double* bS, double* frame_step, double* calib_step);
/* EnergyFunctional::resubstituteF_MT (EnergyFunctional.cpp:272-341) alone, for a caller-supplied x (8nf+4): frame_step (nf*8) and
 * calib_step (4) = -x, the points' steps (resubstituteFPt, :305-341) on the device — sdso_ba_get_point_steps reads them.  Needs the
 * per-point terms of a preceding sdso_ba_accumulate. */
int sdso_ba_resubstitute(sdso_ctx* ctx, int win, const double* x, double* frame_step, double* calib_step);
int sdso_ba_get_point_steps(sdso_ctx* ctx, int win, float* step /* np */);

/* FullSystem::optimize, DSO-native GN loop (FullSystemOptimize.cpp:871-1041, the un-compiled #else):
 * returns final frame states, point idepths and residual states. */
typedef struct {
  int iterations;
  double lastEnergy;      /* lastEnergy[0] */
  double rmse;            /* sqrt(lastEnergy[0]/(patternNum*resInA)) */
  int resInA;
} sdso_ba_opt_result_t;
int sdso_ba_optimize(sdso_ctx* ctx, int win, int mnumOptIts, double* state_out /* nf*10 */,
                     float* idepth_out /* np */, uint8_t* res_state_out /* nr */,
                     sdso_ba_opt_result_t* out);

/* Everything FullSystem::optimize leaves behind in the reference's objects and that its callers read afterwards — the state after
 * the closing `linearizeAll(true)` (FullSystemOptimize.cpp:997-1041 with :52-87 and :142-203) and after the last solveSystemF's
 * AccumulatedSCHessianSSE::addPoint (AccumulatedSCHessian.cpp:34-60).  Valid after sdso_ba_optimize / sdso_ba_batch_optimize[_end]
 * of the window (SDSO_ERR_STATE before).  Every pointer may be NULL; arrays are caller-owned, in the window's point / residual order.
 * Consumers in the reference: CoarseTracker::makeCoarseDepthL0 reads lastResiduals[0].second (= state_state of that residual),
 * centerProjectedTo and efPoint->HdiF (CoarseTracker.cpp:295-350); FullSystem::flagPointsForRemoval reads residuals.size(),
 * isInlierNew() (numGoodResiduals), isOOB() (lastResiduals[].second, maxRelBaseline) and idepth_hessian (FullSystem.cpp:997-1040). */
typedef struct {
  /* per point [np] */
  float* idepth;                 /* PointHessian::idepth (== idepth_zero: doStepFromBackup sets both, :268-272)                       */
  float* step;                   /* PointHessian::step of the last solve                                                              */
  float* HdiF;                   /* EFPoint::HdiF          (AccumulatedSCHessian.cpp:58; 0 when the point had no active residual :44) */
  float* bdSumF;                 /* EFPoint::bdSumF        (:61-65)                                                                   */
  float* idepth_hessian;         /* PointHessian::idepth_hessian (:56; 0 at :46)                                                      */
  float* maxRelBaseline;         /* PointHessian::maxRelBaseline: reset at AccumulatedSCHessian.cpp:47, raised at FullSystemOptimize.cpp:68-74 */
  int* numGoodResiduals;         /* PointHessian::numGoodResiduals after :76                                                          */
  /* per residual [nr] */
  uint8_t* state_state;          /* PointFrameResidual::state_state after applyRes(true); also lastResiduals[k].second (:165-172)     */
  uint8_t* isActiveAndIsGoodNEW; /* EFResidual::isActiveAndIsGoodNEW (Residuals.cpp:367-385)                                          */
  float* state_energy;           /* PointFrameResidual::state_energy                                                                  */
  float* centerProjectedTo;      /* nr*3, meaningful where isActiveAndIsGoodNEW (the final linearisation reached :130-131); else 0    */
  float* projectedTo;            /* nr*16, same rule                                                                                  */
  uint8_t* toRemove;             /* 1: linearizeAll(true) put the residual on toRemove (:80-84) — the caller clears lastResiduals[].first,
                                    calls ef->dropResidual(r->efResidual) and deleteOut(ph->residuals, k) in this order (:176-195)   */
  /* frames */
  double* state;                 /* nf*10  FrameHessian::get_state()                                                                  */
  double* state_zero;            /* nf*10  (the newest frame's changes: setEvalPT at :1000-1003)                                      */
  double* evalPT;                /* nf*12  worldToCam_evalPT: R (9, row-major), t (3); the newest frame's is its PRE_worldToCam        */
  double* PRE_worldToCam;        /* nf*12  (shell->camToWorld = PRE_camToWorld at :1033-1037 is its inverse)                          */
  double* frame_step;            /* nf*10  FrameHessian::step of the last solve                                                       */
  float* frameEnergyTH;          /* nf     (the newest frame's: setNewFrameEnergyTH of the closing linearizeAll)                      */
  /* calibration */
  double calib_value[4];         /* CalibHessian::value (unscaled)                                                                    */
  double calib_value_scaled[4];
  double calib_step[4];
  /* EnergyFunctional members of the last solveSystemF */
  double* lastX;                 /* 8nf+4 */
  double* lastHS;                /* (8nf+4)^2; lastHS / lastbS (log-only in the reference, FullSystem.cpp:1691-1764) are kept by
                                    sdso_ba_optimize; inside a batch only after sdso_ba_batch_keep_system(ctx, 1): SDSO_ERR_STATE otherwise */
  double* lastbS;                /* 8nf+4 */
  int resInA, resInL, resInM;    /* nres of the last accumulateAF / LF; residuals marginalised through this window so far             */
  int n_toRemove;
  sdso_ba_opt_result_t result;   /* what the optimize call returned for this window                                                   */
} sdso_ba_post_state_t;
int sdso_ba_get_post_state(sdso_ctx* ctx, int win, sdso_ba_post_state_t* out);
/* EnergyFunctional::resInA / resInL of the latest accumulate (EnergyFunctional.cpp:219, :241) and resInM: the residuals marginalised
 * through this window by sdso_ba_marginalize_points so far (:704).  Any pointer may be NULL. */
int sdso_ba_get_counts(sdso_ctx* ctx, int win, int* resInA, int* resInL, int* resInM);

/* FullSystem::removeOutliers (FullSystemOptimize.cpp:1063-1084) and FullSystem::flagPointsForRemoval (FullSystem.cpp:965-1056, with
 * PointHessian::isOOB / isInlierNew, HessianBlocks.h:439-469) decided on the device-resident window after an optimize call: one byte
 * per point, nothing per point crosses the bus on the way in.  Per point (csrc/ba_flag.h states the rule once):
 *   n          : its residuals that linearizeAll(true) did not put on toRemove — ph->residuals.size() after FullSystemOptimize.cpp:176-195
 *   n == 0     -> SDSO_PT_DROP_NO_RESIDUAL (removeOutliers);  idepth < 0 -> SDSO_PT_DROP_NEGATIVE (FullSystem.cpp:997)
 *   last[k]    : lastResiduals[k].second, k = 0, 1 = state_state of the point's residual into frame nf-1-k, whether that residual is on
 *                toRemove or not (:167-173 update .second before :184-187 clear .first).  last_gone[2p+k] other than 255 replaces it: the
 *                history of a residual an earlier keyframe dropped.  Neither: ResState::OOB (FullSystemOptPoint.cpp:204-207)
 *   isOOB() || frame_marg[host] -> isInlierNew() ? (idepth_hessian > minIdepthH_marg ? SDSO_PT_MARGINALIZE : SDSO_PT_DROP_WEAK)
 *                                                : SDSO_PT_DROP_NOT_INLIER;  otherwise SDSO_PT_KEEP
 * The re-linearisation and fixLinearizationF of FullSystem.cpp:1012-1021 stay in sdso_ba_marginalize_points.
 *   counts      : points per code.  The reference's statistics follow: flag_nores = [1] + [2], flag_oob = [3] + [4] + [5],
 *                 flag_in = [3] + [4], flag_inin = [3]
 *   host_counts : the same per host frame, [host * 6 + code]: pointHessiansMarginalized grows by code 3, pointHessiansOut by the
 *                 codes 1, 2, 4 and 5 — what the next flagFramesForMarginalization reads
 *   refusals    : decided before any device work.  SDSO_ERR_STATE as for sdso_track_make_ref_from_window: no valid post-state (no
 *                 optimize call has ended on the window, or sdso_ba_window_update has edited it since), a member of a batch, a window
 *                 holding a linearised residual.  SDSO_ERR_ARG: an unknown window, a NULL struct, frame_marg or decision, a last_gone
 *                 byte outside {0, 1, 2, 255}, a negative setting
 * The call changes nothing in the window: a second call returns the same bytes (integer counting only), every getter returns what it
 * returned before.  One upload (last_gone, when given), one kernel, one copy back, one synchronisation. */
#define SDSO_PT_KEEP 0
#define SDSO_PT_DROP_NO_RESIDUAL 1
#define SDSO_PT_DROP_NEGATIVE 2
#define SDSO_PT_MARGINALIZE 3
#define SDSO_PT_DROP_WEAK 4
#define SDSO_PT_DROP_NOT_INLIER 5
typedef struct {
  const uint8_t* frame_marg;      /* nf  FrameHessian::flaggedForMarginalization (flagFramesForMarginalization ran before optimize) */
  const uint8_t* last_gone;       /* np*2 or NULL; 0/1/2 = ResState to use, 255 = derive from the window */
  int   minGoodActiveResForMarg;  /* settings.cpp:82  3  */
  int   minGoodResForMarg;        /* settings.cpp:83  4  */
  float minIdepthH_marg;          /* settings.cpp:57  50 */
} sdso_ba_flag_points_t;
int sdso_ba_flag_points(sdso_ctx* ctx, int win, const sdso_ba_flag_points_t* prm, uint8_t* decision /* np */,
                        int* counts /* 6, per code; may be NULL */, int* host_counts /* nf*6; may be NULL */);

/* EnergyFunctional::marginalizePointsF (EnergyFunctional.cpp:663-736) for the points flagged in
 * marg_flag[np] (after flagPointsForRemoval's linearize + fixLinearizationF, FullSystem.cpp:1012-1021):
 * returns the updated HM / bM. */
int sdso_ba_marginalize_points(sdso_ctx* ctx, int win, const uint8_t* marg_flag, double* HM_out,
                               double* bM_out);

/* EnergyFunctional::marginalizeFrame (EnergyFunctional.cpp:554-660): remove keyframe `idx` (EFFrame::idx) from the
 * marginalisation prior.  prior8 / delta_prior8 are EFFrame::prior / delta_prior.  HM_in (8nf+4)^2, bM_in 8nf+4 ->
 * HM_out (8(nf-1)+4)^2, bM_out.  Host statement of the algebra on caller-owned arrays (no ctx); the device path is
 * sdso_ba_marginalize_frame_dev below. */
int sdso_ba_marginalize_frame(int nf, int idx, const double* prior8, const double* delta_prior8,
                              const double* HM_in, const double* bM_in, double* HM_out, double* bM_out);

/* EnergyFunctional::calcLEnergyF_MT (EnergyFunctional.cpp:420-442; EnergyFunctional.h:82) and calcMEnergyF (:344-351; .h:83) at the
 * window's current state: the values themselves (FullSystem::calcLEnergy / calcMEnergy return 0 under setting_forceAceptStep before
 * they ever call these, FullSystemOptimize.cpp:374-376, :1056).  Either pointer may be NULL. */
int sdso_ba_calc_energies(sdso_ctx* ctx, int win, double* EL, double* EM);
/* What EnergyFunctional::setDeltaF (EnergyFunctional.cpp:173-207; .h:75) leaves behind at the window's current state: cDeltaF (4),
 * EFFrame::delta and delta_prior (nf*8 each), EFPoint::deltaF (np); adHTdeltaF comes with sdso_ba_get_tables.  Any pointer may be NULL. */
int sdso_ba_get_deltas(sdso_ctx* ctx, int win, float* cDeltaF, double* frame_delta, double* frame_delta_prior, float* point_deltaF);

/* The same on the DEVICE-resident prior of an uploaded window: HM / bM as sdso_ba_marginalize_points left them on the device go through
 * the marginalisation of keyframe `idx` in one kernel (its EFFrame::prior / delta_prior are the window's own) and stay there; HM_out
 * (8(nf-1)+4)^2 / bM_out are optional host copies.  sdso_ba_adopt_prior(win, from_win) hands that prior to the next window — device to
 * device, the rows / columns of frames beyond it zero, as EnergyFunctional::insertFrame resizes HM / bM (EnergyFunctional.cpp:468-476);
 * upload `win` with HM = bM = NULL first.  The prior then never leaves the device between two keyframes.
 * Several frames leaving at one keyframe (FullSystem.cpp:1470-1476 marginalises every flagged frame in a loop): a call that follows another
 * one with no sdso_ba_marginalize_points in between continues from that result, `idx` then counting the frames the prior still covers
 * (EFFrame::idx after the earlier frame was erased); outputs are (8k+4)^2 / 8k+4 for the k frames left.  sdso_ba_adopt_prior fails (-1)
 * unless the adopting window's leading frames are exactly those k frames, in order (by frameID), and it was uploaded with a zero prior. */
int sdso_ba_marginalize_frame_dev(sdso_ctx* ctx, int win, int idx, double* HM_out, double* bM_out);
int sdso_ba_adopt_prior(sdso_ctx* ctx, int win, int from_win);

/* Edit an uploaded window IN PLACE: the device form of EnergyFunctional::insertResidual (EnergyFunctional.cpp:445), insertFrame (:462),
 * insertPoint (:507), dropResidual (:524), dropPointsF (:739), removePoint (:755), the removePoint loop of marginalizePointsF (:692-696)
 * and the residual drops of FullSystem::marginalizeFrame (FullSystemMarginalize.cpp:146-198).  The seven stages run in this order; every
 * index of an existing frame / point / residual refers to the window BEFORE the call (an appended frame k is nf_before + k).  Any stage
 * may be empty.  Afterwards the window is what sdso_ba_upload_window of the edited window would have made (makeIDX order, :998-1018),
 * with every float-valued state of the surviving points and residuals carried on the device:
 *   carried (device)     : u, v, idepth, idepth_zero, colour, weights, maxRelBaseline, numGoodResiduals, res_state, isNew
 *   carried (host mirror): calibration, frame states / evalPT / frameEnergyTH / exposure / frameID / slot, hasDepthPrior, solverMode,
 *                          affine modes, forceAcceptStep, resInM
 *   prior                : no frame leaves: HM / bM as the device holds them, the rows / columns of appended frames zero (insertFrame,
 *                          :476-482).  Frames leave: the caller has run sdso_ba_marginalize_frame_dev for exactly those frames since the
 *                          last sdso_ba_marginalize_points; that chained prior is installed device to device.
 *   everything else      : as after an upload (no post-state, nothing linearised, accumulators cleared). */
typedef struct {
  /* stage 1  dropResidual (:524-533), one after the other in the given order: the LAST entry of residualsAll takes the freed slot */
  int n_drop_res;      const int* drop_res;
  /* stage 2  removePoint (:755-771) one after the other in the given order: marginalizePointsF's loop over allPointsToMarg (:692-696) */
  int n_remove_points; const int* remove_points;
  /* stage 3  dropPointsF (:739-752): per host frame the rescanning loop `if flagged: removePoint, i--` */
  const uint8_t* drop_point;                        /* np flags, or NULL */
  /* stage 4  frames leave, one after the other (FullSystemMarginalize.cpp:146-198): every remaining point drops its residual into that
   *          frame (swap-with-last), then the frame is erased and later frames move up */
  int n_remove_frames; const int* remove_frames;
  /* stage 5  insertFrame (:462-504): appended at the end */
  int n_add_frames;
  const double* evalPT; const double* state; const double* state_zero;      /* as in sdso_ba_window_t, n_add_frames entries */
  const float* ab_exposure; const float* frameEnergyTH; const int* frameID; const int* frame_slot;
  /* stage 6  insertResidual (:445-458) on surviving points: pushed to the back of residualsAll in the given order */
  int n_add_res; const int* add_res_point; const int* add_res_target;
  const uint8_t* add_res_state; const uint8_t* add_res_isNew;               /* isNew NULL: 1 */
  /* stage 7  insertPoint (:507-521): pushed to the back of its host's list in the given order, with its residuals */
  int n_add_points;
  const int* pt_host;                               /* may be an appended frame */
  const float* pt_u; const float* pt_v; const float* pt_idepth; const float* pt_idepth_zero;
  const float* pt_color; const float* pt_weights;   /* n_add_points*8 */
  const uint8_t* pt_hasDepthPrior; const float* pt_maxRelBaseline; const int* pt_numGoodResiduals;   /* the last two NULL: 0 */
  int n_pt_res; const int* pt_res_point;            /* index into the appended points, non-decreasing */
  const int* pt_res_target; const uint8_t* pt_res_state; const uint8_t* pt_res_isNew;                /* isNew NULL: 1 */
} sdso_ba_window_edit_t;
/* The order the edit produces, on the host without a ctx (like sdso_ba_marginalize_frame).
 *   in : nf, np, nr, host[np], res_point[nr], res_target[nr] of the window before the edit
 *   out: nf2 / np2 / nr2 and, each optional, frame_src[nf2], point_src[np2], res_src[nr2]: the index before the edit, or -1-k for the
 *        k-th appended frame / point / residual (stage 6's residuals first, then stage 7's).  Size the arrays for nf + n_add_frames,
 *        np + n_add_points, nr + n_add_res + n_pt_res.
 * SDSO_ERR_ARG for an edit the reference could not perform: an index out of range or named twice in one stage; a point or residual
 * named after an earlier stage removed it; a residual added to a point that leaves, onto its own host, onto a target the point already
 * observes, as a ninth residual, or into a frame that leaves; a frame leaving that still hosts a point
 * (assert(frame->pointHessians.size()==0), FullSystemMarginalize.cpp:148); more than 8 frames. */
int sdso_ba_window_plan(int nf, int np, int nr, const int* host, const int* res_point, const int* res_target,
                        const sdso_ba_window_edit_t* E, int* nf2, int* np2, int* nr2,
                        int* frame_src, int* point_src, int* res_src);
/* Apply the edit (enqueue only, like sdso_ba_upload_window).  Every refusal is decided before any device work and leaves the window as it
 * was: SDSO_ERR_ARG as for sdso_ba_window_plan or for an appended frame without an uploaded pyramid of the window's size; SDSO_ERR_STATE
 * for a window inside a batch (sdso_ba_batch_create again afterwards), a surviving residual that is linearised (fixLinearizationF only
 * touches points that leave), a frame removal without the matching sdso_ba_marginalize_frame_dev calls, and an edit that removes no
 * frame after sdso_ba_marginalize_frame_dev has run (its prior would be lost). */
int sdso_ba_window_update(sdso_ctx* ctx, int win, const sdso_ba_window_edit_t* E);
/* sdso_ba_window_update with stage 7 taken from the latest sdso_imm_activate of this ctx, device to device: the tail of
 * optimizeImmaturePoint (FullSystemOptPoint.cpp:196-237) and STEP 4 of activatePointsMT (FullSystem.cpp:919-945) on the resident window.
 * Stages 1-6 of E are as above; stage 7 of E must be empty (n_add_points == n_pt_res == 0, else SDSO_ERR_ARG).
 *   appended points : toOptimize is walked in order; every entry with status 1 is one point, in that order (FullSystem.cpp:923-928
 *                     `newpoint != 0 && newpoint != -1`; the non-finite energyTH of FullSystemOptPoint.cpp:199-202 is already status -1)
 *       host                 act_frame[rec.frame]                      (HessianBlocks.cpp:37 `host = rawPoint->host`)
 *       u, v, colour, weights   the record's                           (HessianBlocks.cpp:45-46, :60-61)
 *       idepth, idepth_zero  both rec.idepth                           (FullSystemOptPoint.cpp:208-209 setIdepthZero / setIdepth(currentIdepth))
 *       hasDepthPrior, maxRelBaseline, numGoodResiduals   0            (HessianBlocks.cpp:38, :41-42)
 *   their residuals : for f = 0 .. nf_act-1 in the activation's frame order, rec.res_state[f] == IN is one residual with target
 *                     act_frame[f], state IN, isNew 1 (FullSystemOptPoint.cpp:213-219; FullSystem.cpp:931-932 inserts them in that order;
 *                     the host's own entry is 255 and gives none)
 *   act_frame       : nf of the activation entries, the window frame of every activation frame in the edit's convention: an index of the
 *                     window before the call, nf_before + k for the k-th appended frame.  The appended residuals follow stage 6's in
 *                     res_src, as stage 7's do in sdso_ba_window_update.
 *   n_points, n_res : the numbers appended (each may be NULL)
 *   act_index       : act_index[k] = the toOptimize index of the k-th appended point (may be NULL; size it for counts[4] of the activation)
 * The host reads the integer members of the records (frame, status, res_state), plans the edit as sdso_ba_window_plan does and stages the
 * integers; the float rows of the appended points are filled from the records on the device.  No float of an activated point is read
 * from or written to host memory.  Enqueue only.  sdso_ba_window_get_order works as after any update.
 * Refused before any device work, the window, the set and the records left as they were:
 *   SDSO_ERR_STATE  no sdso_imm_activate on this ctx yet; its result was already taken by an earlier successful call of this function
 *                   (every sdso_imm_activate makes a fresh one); everything sdso_ba_window_update refuses with this code
 *   SDSO_ERR_ARG    null act_frame; an entry out of range of the edited window or naming a frame that leaves in stage 4; two activation
 *                   frames mapped to one window frame; the activation's w x h other than the window's; everything sdso_ba_window_plan
 *                   refuses
 * A call with no activated point is a plain update; it consumes the (empty) result all the same. */
int sdso_ba_window_update_activated(sdso_ctx* ctx, int win, const sdso_ba_window_edit_t* E, const int* act_frame,
                                    int* n_points, int* n_res, int* act_index);
/* The maps of the latest sdso_ba_window_update of this window (sizes: its current nf / np / nr; each may be NULL); SDSO_ERR_STATE when
 * the window has not been updated since its upload. */
int sdso_ba_window_get_order(sdso_ctx* ctx, int win, int* frame_src, int* point_src, int* res_src);

/* keep projectedTo / centerProjectedTo of PointFrameResidual (Residuals.h:96-99) for
 * sdso_ba_get_linearization; off by default (76 B of extra stores per residual). */
int sdso_ba_keep_projections(sdso_ctx* ctx, int win, int on);

/* Batches: any number of uploaded windows (same nf) advance through one GN iteration with ONE
 * launch per phase.  The packed accumulators of the batch are contiguous so that one RCCL
 * all-reduce over xGMI covers every window when the points of each window are sharded across
 * ranks:
 *   sdso_ba_batch_accumulate : linearizeAll + applyRes + accumulateAF/LF/SCF      (enqueue only)
 *   [all-reduce(sum) of sdso_ba_batch_accum_dev across ranks]
 *   sdso_ba_batch_solve      : stitch + solveSystemF + resubstituteF              (enqueue only)
 *   sdso_ba_batch_get_x      : lastX of every window (synchronises)
 * Windows in the SOLVER_SVD / SOLVER_ORTHOGONALIZE_SYSTEM modes (EnergyFunctional.cpp:876-900, 924-965) run on the device like the others
 * (one workgroup per window: projected system, parallel-order Jacobi eigen-decomposition or the pivoted LDL^T; enqueue only, resident
 * loop included); the members of a batch share one solver branch. */
int sdso_ba_batch_create(sdso_ctx* ctx, int nwin, const int* wins);
int sdso_ba_batch_accumulate(sdso_ctx* ctx);
/* = sdso_ba_batch_linearize (linearizeAll + applyRes + accumulateAF) followed by sdso_ba_batch_schur (accumulateLF/SCF + folds),
 * available separately for callers that interleave several batches on several contexts / streams */
int sdso_ba_batch_linearize(sdso_ctx* ctx);
int sdso_ba_batch_schur(sdso_ctx* ctx);
/* 1 (default): every linearization writes the RawResidualJacobian records to HBM like
 * PointFrameResidual::J; 0: they stay in registers of the fused linearize+accumulate kernel. */
int sdso_ba_batch_set_materialize(sdso_ctx* ctx, int materialize);
/* 1: every solve of the batch's resident loop also writes EnergyFunctional::lastHS / lastbS (EnergyFunctional.cpp:909-910; log-only in
 * the reference) so that sdso_ba_get_post_state can return them; 0 (default): they are not materialised (37 KB per window and iteration). */
int sdso_ba_batch_keep_system(sdso_ctx* ctx, int on);
/* Shape of the exchange of a SHARDED batch inside the resident loop (points of every window cut over the ranks of the ctx's
 * communicator; the accumulators are sums over points like the reference's per-thread copies, AccumulatedTopHessian.cpp:299-308):
 *   0 (default)  sdso_ba_allreduce = one all-reduce of the packed block; every rank stitches and solves every window;
 *   1            sdso_ba_allreduce = one reduce-scatter by window (rank r receives the sums of windows [r*nwin/N, (r+1)*nwin/N)), the
 *                solve of a window runs on that rank only, and x / xAd / nres of every window go round by one all-gather
 *                (136 + 8 nf^2 + 2 floats per window) inside sdso_ba_batch_solve_step: half the xGMI bytes per link.
 * Mode 1 applies when nwin divides by the ranks, the loop is the accepted-step flow and lastHS / lastbS are not kept; otherwise the call
 * falls back to the all-reduce.  The results are the same bits either way (the sums are the same numbers). */
int sdso_ba_batch_exchange_mode(sdso_ctx* ctx, int mode);
/* lambda is subject to the windows' solverMode exactly as in solveSystemF (SOLVER_USE_GN -> 0, SOLVER_FIX_LAMBDA -> 1e-5,
 * EnergyFunctional.cpp:840-846); the members of a batch must share one solverMode. */
int sdso_ba_batch_solve(sdso_ctx* ctx, double lambda, int orthogonalize_x);
int sdso_ba_batch_accum_dev(sdso_ctx* ctx, void** dev_ptr, long* nfloats);
int sdso_ba_batch_get_x(sdso_ctx* ctx, double* x /* nwin*(8nf+4) */);
/* EnergyFunctional::accumulateAF_MT / accumulateLF_MT / accumulateSCF_MT (EnergyFunctional.cpp:212-269) as the reference's callers see
 * them: the STITCHED systems (AccumulatedTopHessianSSE::stitchDoubleMT without / with priors, AccumulatedTopHessian.h:95-148;
 * AccumulatedSCHessianSSE::stitchDoubleMT, AccumulatedSCHessian.h:96-135) of the accumulators sdso_ba_accumulate left: (8nf+4)^2
 * row-major + (8nf+4) doubles each, any pointer may be NULL.  solveSystemF adds them up (:856-868); the fused kernels never
 * materialise them, this call runs the stitch kernels on demand (synchronises).  Right after sdso_ba_marginalize_points the same call
 * returns what marginalizePointsF stitches (EnergyFunctional.cpp:707-717): HA / bA = M, Mb of accSSE_top_A->stitchDouble(.., false, false)
 * over addPoint<2> of the flagged points, Hsc / bsc = Msc, Mbsc. */
int sdso_ba_get_stitched(sdso_ctx* ctx, int win, double* HA, double* bA, double* HL, double* bL, double* Hsc, double* bsc);

/* FullSystem::optimize (FullSystemOptimize.cpp:871-1041, DSO-native loop) for EVERY window of the batch, device-resident: the host
 * logic between the kernel phases — backupState / doStepFromBackup (:207-351), FrameHessian::setState, setPrecalcValues
 * (HessianBlocks.cpp:206-242), setDeltaF (EnergyFunctional.cpp:173-207), setNewFrameEnergyTH (:98-139), the break test — runs in one
 * workgroup per window (k_ba_opt_step), so a whole loop is enqueued without a host round trip.  The accepted-step flow
 * (setting_forceAceptStep = true, the reference's default, settings.cpp:53) runs through the fused linearise+accumulate kernel; with
 * forceAcceptStep = 0 the energy gate of :961-990 (calcLEnergy, calcMEnergy, accept or loadSateBackup + re-linearisation, lambda * 0.25 /
 * * 100) is taken on the device too (k_ba_opt_gate; single rank, sdso_ba_batch_optimize only).  The members of a batch share
 * forceAcceptStep.
 *   sdso_ba_batch_optimize       : the whole loop with the reference's lambda (1e-1 * 0.25^it, subject to solverMode) and
 *                                  orthogonalisation schedule; out[nwin].  With a communicator on ctx (points sharded over ranks) every
 *                                  iteration all-reduces the accumulators and all-gathers the newest-frame energies / break-test sums, so
 *                                  every rank takes the decisions of the unsharded window.
 *   ..._begin / sdso_ba_batch_step / ..._end : the same in pieces, for callers that drive the iterations themselves:
 *       begin ; per iteration { sdso_ba_batch_accumulate ; [sdso_ba_allreduce] ; sdso_ba_batch_solve ; sdso_ba_batch_step } ; end
 *     stop_on_convergence = 0 keeps every window iterating (benchmarks).
 *   sdso_ba_batch_solve_step     : sdso_ba_batch_solve + sdso_ba_batch_step as ONE enqueue — EnergyFunctional::solveSystemF (:838-995),
 *                                  resubstituteF (:272-341), doStepFromBackup, setPrecalcValues, setDeltaF, setNewFrameEnergyTH and the
 *                                  break test in one launch of the fused tail kernel (k_ba_tail: a persistent workgroup per window;
 *                                  the stitched system never leaves the CU).  lambda / orthogonalize_x as in sdso_ba_batch_solve.
 *   sdso_ba_get_state            : states / idepths / residual states of one window as they stand (synchronises). */
int sdso_ba_batch_optimize(sdso_ctx* ctx, int mnumOptIts, sdso_ba_opt_result_t* out /* nwin */);
int sdso_ba_batch_optimize_begin(sdso_ctx* ctx, int stop_on_convergence);
int sdso_ba_batch_step(sdso_ctx* ctx);
int sdso_ba_batch_solve_step(sdso_ctx* ctx, double lambda, int orthogonalize_x);
int sdso_ba_batch_optimize_end(sdso_ctx* ctx, sdso_ba_opt_result_t* out /* nwin, may be NULL */);
int sdso_ba_get_state(sdso_ctx* ctx, int win, double* state_out /* nf*10 */, float* idepth_out /* np */, uint8_t* res_state_out /* nr */);

/* ------------------------------------------------------------------ multi-GPU exchange
 * The points of every window are sharded over the ranks (one process per GPU, contiguous allPoints ranges, every rank holds all
 * pyramids and frame states); the packed accumulators are plain sums over points — the reference adds the per-thread copies the same
 * way before it stitches (AccumulatedTopHessian.cpp:299-308, AccumulatedSCHessian.cpp:136-185) — so ONE all-reduce(sum, float32) per
 * Gauss-Newton iteration over RCCL / xGMI makes every rank stitch and solve the same system:
 *     sdso_ba_batch_accumulate -> sdso_ba_allreduce -> sdso_ba_batch_solve           (all three only enqueue on the ctx stream)
 * RCCL is loaded (dlopen) by the first of these calls; single-GPU users never need it.
 *   sdso_comm_unique_id : rank 0 creates the 128-byte ncclUniqueId; the caller ships it to the other ranks (MPI, sockets, a file ...)
 *   sdso_comm_init      : collective over the nranks processes; binds the communicator to ctx (its device, its stream)
 *   sdso_comm_attach    : a second ctx of the same process / device uses the communicator of `owner`
 *                         (`owner` must not be re-initialised or destroyed concurrently with this call)
 *   sdso_ba_allreduce   : in-place sum of the batch's contiguous block (sdso_ba_batch_accum_dev) over the ranks
 *   sdso_ba_allreduce_window : the same for one window's block (sdso_ba_accum_dev), between sdso_ba_accumulate and sdso_ba_solve
 * A single-iteration exchange sums everything solveSystemF needs.  The energy threshold of the newest frame (setNewFrameEnergyTH,
 * FullSystemOptimize.cpp:98-139: a 70 % quantile over its residuals) is NOT additive: a multi-iteration loop over sharded points has to
 * gather those energies as well — sdso_ba_batch_optimize / sdso_ba_batch_step do (one all-gather per iteration); sdso_ba_optimize is a
 * single-rank call. */
int sdso_comm_unique_id(void* id128);
int sdso_comm_init(sdso_ctx* ctx, int nranks, int rank, const void* id128);
int sdso_comm_attach(sdso_ctx* ctx, sdso_ctx* owner);
/* The same communicator over a transport of the caller's (MPI, sockets, a test harness) instead of RCCL: the library stages each
 * collective through host memory and calls allreduce (in-place sum of n floats) / allgather (n floats per rank, rank-major into recv);
 * both return 0 on success.  Slow path by construction (it synchronises the ctx stream around every collective). */
typedef int (*sdso_host_allreduce_fn)(void* user, float* buf, size_t n);
typedef int (*sdso_host_allgather_fn)(void* user, const float* send, float* recv, size_t n);
int sdso_comm_init_host(sdso_ctx* ctx, int nranks, int rank, sdso_host_allreduce_fn allreduce, sdso_host_allgather_fn allgather, void* user);
int sdso_comm_info(sdso_ctx* ctx, int* nranks, int* rank);   /* nranks = 0 without a communicator */
int sdso_comm_destroy(sdso_ctx* ctx);
int sdso_ba_allreduce(sdso_ctx* ctx);
int sdso_ba_allreduce_window(sdso_ctx* ctx, int win);

/* host tables derived from the frame states (tests): precalc nf*nf*27 floats per (host*nf+target)
 * {PRE_KRKiTll 9, PRE_KtTll 3, PRE_RTll_0 9, PRE_tTll_0 3, PRE_aff_mode 2, PRE_b0_mode 1}
 * (FrameFramePrecalc::set, HessianBlocks.cpp:206-242); adHost/adTarget nf*nf*64 doubles and
 * adHTdeltaF nf*nf*8 floats indexed h+t*nf (EnergyFunctional.cpp:41-119, :173-207). */
int sdso_ba_get_tables(sdso_ctx* ctx, int win, float* precalc, double* adHost, double* adTarget,
                       float* adHTdeltaF);

/* ------------------------------------------------------------------ static stereo
 * ImmaturePoint::ImmaturePoint (src/FullSystem/ImmaturePoint.cpp:33-62) for n pixels of a frame:
 * color[n*8], weights[n*8], gradH[n*4], energyTH[n] (NaN marks a rejected point). */
int sdso_immature_init_batch(sdso_ctx* ctx, int frame_slot, int n, const float* u, const float* v,
                             float* color, float* weights, float* gradH, float* energyTH);

/* in/out point state of ImmaturePoint::traceStereo (ImmaturePoint.h:60-102), SoA */
typedef struct {
  int n;
  float* u_stereo; float* v_stereo;
  float* idepth_min; /* the (unused by stereo) temporal idepth_min tested at ImmaturePoint.cpp:195 */
  float* idepth_min_stereo; float* idepth_max_stereo; float* idepth_stereo;
  float* color;      /* n*8 */
  float* weights;    /* n*8 */
  float* gradH;      /* n*4 */
  float* energyTH;
  float* quality;
  uint8_t* lastTraceStatus;     /* ImmaturePointStatus, in/out */
  float* lastTraceUV;           /* n*2 */
  float* lastTracePixelInterval;
} sdso_trace_points_t;

/* ImmaturePoint::traceStereo (ImmaturePoint.cpp:94-451) for every point; the sub-pixel GN is the
 * DSO-native one (twin at :707-769).  K = {fx,fy,cx,cy}. status[n] = returned ImmaturePointStatus. */
int sdso_trace_stereo_batch(sdso_ctx* ctx, int frame_slot, const float K[4], float baseline,
                            int mode_right, sdso_trace_points_t* pts, uint8_t* status);
/* The same in three steps, for callers that keep the point state resident in HBM:
 * prepare uploads it once, enqueue launches the trace (no copy, no sync; may be repeated),
 * fetch copies the in/out fields and the returned statuses back. */
int sdso_trace_stereo_prepare(sdso_ctx* ctx, int frame_slot, const float K[4], float baseline,
                              int mode_right, const sdso_trace_points_t* pts);
int sdso_trace_stereo_enqueue(sdso_ctx* ctx);
int sdso_trace_stereo_fetch(sdso_ctx* ctx, sdso_trace_points_t* pts, uint8_t* status);

/* PixelSelector::makeMaps (src/FullSystem/PixelSelector2.cpp:193-300, with makeHists :84-189 and select :330-540): candidate
 * pixels of the keyframe in `frame_slot` (needs pyramid levels 0..2; absSquaredGrad = dx*dx + dy*dy, identity response).
 *   potential : PixelSelector::currentPotential, in/out (3 after construction)
 *   map_out   : w*h floats, 0 / 1 / 2 / 4 = not selected / selected at level 0 / 1 / 2   (may be NULL)
 *   num_out   : the value makeMaps returns (points left after the random thinning)
 * The random pattern is glibc's rand() & 0xFF after srand(3141592) (:43-44), reproduced inside the library. */
int sdso_pixel_select(sdso_ctx* ctx, int frame_slot, float density, int recursionsLeft, float thFactor,
                      int* potential, float* map_out, int* num_out);
int sdso_pixel_selector_pattern(int n, unsigned char* out); /* host only: first n pattern bytes */

/* ImmaturePoint::traceOn (ImmaturePoint.cpp:459-828): the temporal epipolar search of every immature point of every host
 * keyframe in the newest frame (FullSystem::traceNewCoarseKey / NonKey, FullSystem.cpp:632-790).  geom[g] is the
 * hostToFrame geometry of host g (:654-665): KRKi = K R K^-1, Kt = K t, aff = AffLight::fromToVecExposure(...) as floats;
 * point_geom[i] selects it.  pts uses the traceStereo layout with u_stereo/v_stereo = u/v and idepth_min_stereo /
 * idepth_max_stereo = idepth_min / idepth_max (in/out); idepth_min and idepth_stereo are not used. */
typedef struct { float KRKi[9]; float Kt[3]; float aff[2]; } sdso_trace_geom_t;
int sdso_trace_on_batch(sdso_ctx* ctx, int frame_slot, int ngeom, const sdso_trace_geom_t* geom, const int* point_geom,
                        sdso_trace_points_t* pts, uint8_t* status);

/* FullSystem::optimizeImmaturePoint (FullSystemOptPoint.cpp:52-238) with ImmaturePoint::linearizeResidual
 * (ImmaturePoint.cpp:886-985), the DSO-native idepth-only Gauss-Newton, for n candidate points at once
 * (FullSystem::activatePointsMT, FullSystem.cpp:796-958).  pair_* are the FrameFramePrecalc members the reference reads
 * (host->targetPrecalc[target->idx]: PRE_RTll, PRE_tTll, PRE_aff_mode), indexed host*nf+target.
 *   status[n]      : 1 activated, 0 not well-constrained (the reference returns 0), -1 outlier (returns (PointHessian*)-1)
 *   idepth_out[n]  : currentIdepth at exit
 *   res_state[n*nf]: final ResState per target frame (255 for the host itself / not evaluated) */
typedef struct {
  int nf, w, h, n, minObs;
  float K[4];                              /* fxl fyl cxl cyl */
  const float* pair_R; const float* pair_t; const float* pair_aff;
  const int* frame_slot;                   /* nf pyramid slots */
  const float* const* dI;                  /* unused by the library (layout shared with the test oracle) */
  const int* host; const float* u; const float* v; const float* idepth_min; const float* idepth_max;
  const float* color; const float* weights; const float* energyTH;
} sdso_activate_t;
int sdso_activate_points_batch(sdso_ctx* ctx, const sdso_activate_t* A, int8_t* status, float* idepth_out, uint8_t* res_state);

/* CoarseDistanceMap (src/FullSystem/CoarseTracker.h:165-197) and the first half of FullSystem::activatePointsMT
 * (FullSystem.cpp:823-902): the step between sdso_trace_on_batch and sdso_activate_points_batch.  One map per ctx, at pyramid
 * level 1 (w1 = w >> 1, h1 = h >> 1), resident on the device; values are 0..39 (the growth step that reached the pixel) or 1000.
 *
 * sdso_distmap_make = CoarseDistanceMap::makeDistanceMap (CoarseTracker.cpp:1216-1255) + growDistBFS (:1260-1363).
 *   geom[g]   : K[1] * fhToNew.rotationMatrix().cast<float>() * Ki[0] and K[1] * fhToNew.translation().cast<float>() of keyframe g as
 *               the caller computes them at :1235-1236; point_geom[i] selects it
 *   u, v, idepth_scaled : PointHessian members of the n active points, in the reference's loop order
 *   n_seeds   : numItems — the projections inside 0 < u < w1, 0 < v < h1, duplicates counted (may be NULL)
 * A projection whose quotient is not finite or does not fit an int (undefined in the reference) counts as outside the image.
 * sdso_distmap_add = CoarseDistanceMap::addIntoDistFinal(u, v) (:1366-1372) for n pixels one after the other, in order.
 * sdso_distmap_get = fwdWarpedIDDistFinal, w1*h1 floats.
 * add / get / sdso_activate_select return SDSO_ERR_STATE until a map has been made on this ctx. */
typedef struct { float KRKi[9]; float Kt[3]; } sdso_distmap_geom_t;
int sdso_distmap_make(sdso_ctx* ctx, int w, int h, int ngeom, const sdso_distmap_geom_t* geom, int n, const int* point_geom,
                      const float* u, const float* v, const float* idepth_scaled, int* n_seeds);
/* sdso_distmap_make on the points of the device-resident BA window `win`, read where they lie: point p of host frame f is projected with
 * geom[f], its u, v and its current idepth — the value sdso_ba_get_state returns (idepth_scaled, SCALE_IDEPTH = 1).
 *   geom : one entry per frame of the window (fhToNew of :1235-1236); skip : nf flags or NULL — the points of a frame with skip[f] != 0
 *          contribute nothing (`if (fh == frame) continue`, CoarseTracker.cpp:1232, when the newest frame is already in the window)
 * The window's own point order stands in for "the reference's loop order": every seed stores the same 0 and numItems only counts them, so
 * the map does not depend on the order of the points (and the window keeps the reference's order anyway, makeIDX).
 * Only geom and skip travel to the device.  With n_seeds == NULL the call does not synchronise.
 * SDSO_ERR_ARG, decided before any device work (the previous map stays valid): an unknown window, w / h other than the window's, null geom. */
int sdso_distmap_make_from_window(sdso_ctx* ctx, int win, int w, int h, const sdso_distmap_geom_t* geom, const uint8_t* skip, int* n_seeds);
int sdso_distmap_add(sdso_ctx* ctx, int n, const int* iu, const int* iv);
int sdso_distmap_get(sdso_ctx* ctx, float* map /* w1*h1 */);

/* FullSystem::activatePointsMT STEP 2 (FullSystem.cpp:837-902) for the n immature points of every keyframe but the newest, flattened
 * in the reference's loop order (hosts in frameHessians order, each host's immaturePoints in index order).  Works on the map the
 * preceding sdso_distmap_make left in the ctx and leaves the re-grown map there (every selection runs addIntoDistFinal, :893, so a
 * candidate is tested against the points selected before it).
 *   geom[g], host_flagged[g] : KRKi / Kt (:841-842) and FrameHessian::flaggedForMarginalization of host g; point_geom[i] selects it
 *   lastTraceStatus          : ImmaturePointStatus (ImmaturePoint.h:50-56)
 *   decision[n]   : 0 KEEP (stays immature), 1 DELETE (`delete ph; host->immaturePoints[i] = 0`), 2 SELECT (pushed to toOptimize)
 *   iu, iv [n]    : the level-1 pixel of :884-885, valid where the candidate reached the distance test (SELECT, or KEEP by
 *                   distance); unspecified elsewhere; may be NULL
 *   n_selected    : toOptimize.size() (may be NULL) */
typedef struct {
  int w, h;                                /* wG[0], hG[0] */
  int ngeom;
  const sdso_distmap_geom_t* geom;         /* ngeom */
  const uint8_t* host_flagged;             /* ngeom */
  int n;
  const int* point_geom;
  const float* u; const float* v; const float* idepth_min; const float* idepth_max;
  const float* quality; const float* lastTracePixelInterval;
  const uint8_t* lastTraceStatus;
  const float* my_type;
  float currentMinActDist;                 /* FullSystem::currentMinActDist after STEP 1 (:798-817) */
  float minTraceQuality;                   /* setting_minTraceQuality = 3 (settings.cpp:112) */
} sdso_activate_select_t;
int sdso_activate_select(sdso_ctx* ctx, const sdso_activate_select_t* S, uint8_t* decision, int* iu, int* iv, int* n_selected);

/* Left-right-left matching as every caller of traceStereo performs it (FullSystem::stereoMatch FullSystem.cpp:581-613,
 * traceNewCoarseNonKey :667-725, CoarseTracker::makeCoarseDepthL0 CoarseTracker.cpp:295-347):
 *   forward: ImmaturePoint(u, v, frame A) traced into frame B   (interval idepth_min/max_stereo, NULL = fresh 0 / NaN)
 *   back   : where the forward trace is IPS_GOOD, ImmaturePoint(lastTraceUV, frame B) traced into frame A
 * The accept rule differs per caller (|u - back_uv[0]| < 1 and a depth bound), so it is left to the caller.
 * status_back is 255 where the back trace did not run.  Any output pointer may be NULL. */
typedef struct {
  int n;
  const float* u; const float* v;
  const float* idepth_min_stereo; const float* idepth_max_stereo;
  const float* back_idepth_min_stereo; const float* back_idepth_max_stereo;
  uint8_t* status_fwd; uint8_t* status_back;
  float* idepth_stereo; float* idepth_min_out; float* idepth_max_out;   /* of the forward trace */
  float* fwd_uv;   /* n*2 lastTraceUV of the forward trace */
  float* back_uv;  /* n*2 lastTraceUV of the back trace */
} sdso_stereo_match_t;
int sdso_stereo_match_batch(sdso_ctx* ctx, int slot_a, int slot_b, const float K[4], float baseline,
                            int mode_right_first, sdso_stereo_match_t* m);

/* ------------------------------------------------------------------ the stereo initialiser
 * The start of a sequence: the live part of CoarseInitializer::setFirstStereo (src/FullSystem/CoarseInitializer.cpp:838-1034, called at
 * FullSystem.cpp:1092-1093) and STEP 3 of FullSystem::initializeFromInitializer (FullSystem.cpp:1487-1597, called from trackNewCoarse at
 * :309).  One initialiser state per ctx, with buffers of its own: no other entry point reads or writes them, and these calls touch
 * neither the resident immature set nor the batches of the other stereo entry points.
 * Not built, because nothing live reads it: levels >= 1 (makePixelStatus and the idepth[lvl] sums, CoarseInitializer.cpp:975-1013), makeNN
 * (:1249), dGrads, setFirst, trackFrame and calcResAndGS.  Their only reader is the monocular trackFrame, which this fork never calls;
 * the uses outside the class (FullSystem.cpp:1092-1093 and :1498-1576) touch points[0] / numPoints[0] only.
 *
 * sdso_init_set_first_stereo = setFirstStereo, level 0 (CoarseInitializer.cpp:842-972).  For y in [3, h-4), x in [3, w-4) in raster order
 * every pixel with map != 0 becomes one Pnt: ImmaturePoint(x, y, firstFrame, map[i]) (ImmaturePoint.cpp:33-62) with u_stereo = u,
 * v_stereo = v, idepth_min_stereo = 0, idepth_max_stereo = NaN, traced by traceStereo(right_slot, K, 1) (:897-903) in the ctx's refinement
 * mode (sdso_trace_set_gn_mode).  IPS_GOOD: idepth = iR = idepth_stereo (:905-911); any other status: idepth = iR = 0.01f (:942-947);
 * both branches: u = x, v = y, my_type = map[i].  isGood = true and outlierTH = patternNum * setting_outlierTH are the same for every
 * Pnt and not stored.  Unlike makeNewTraces (sdso_imm_add_frame), a point whose energyTH is not finite is NOT dropped.  Such a point (a
 * NaN among its colours) has no best search step, and the reference then refines around (0, 0), reading in front of the image; its
 * status does not depend on what it reads (ImmaturePoint.cpp:413 holds for a NaN energyTH).  Here it takes no search and gets that
 * status: IPS_OOB where the search line fails its tests (:118-238), IPS_OUTLIER otherwise; its interval stays 0 / NaN.  What the caller
 * sets afterwards (:1027-1029: thisToNext = SE3(), snapped = false, frameID = snappedAt = 0) stays with the caller.
 *   selection_map : w*h host floats, or NULL = PixelSelector::makeMaps(firstFrame, statusMap, 0.03f*w*h, 1, false, 2) with a fresh
 *                   currentPotential of 3 (:848-871), run by the library on frame_slot as sdso_pixel_select does; that map then is "the
 *                   map of the latest sdso_pixel_select" of this ctx
 *   numPoints     : numPoints[0], the number of Pnts.  It can be smaller than makeMaps' return value: selected pixels in the excluded
 *                   border are skipped
 *   counts        : SDSO_INIT_NCOUNTS ints: [0] non-zero map entries (= makeMaps' return value when the library selected), [1]
 *                   numPoints[0], [2..7] the histogram of the returned ImmaturePointStatus 0..5 over the Pnts
 * Copies nothing up except a caller-supplied map.  With its own map the call reads the candidate count back once to size its launches
 * (sdso_pixel_select synchronises as well); with a caller's map nothing is waited for unless counts is given, which copies the counts
 * back: numPoints == NULL and counts == NULL only enqueue.  The call replaces an earlier state of this ctx.  A map with no entry in the
 * walked area is not an error: the counts are 0 and n = 0.
 * Refused before any device work, an earlier state left as it was: SDSO_ERR_ARG for an unknown frame_slot or right_slot, a right pyramid
 * of another size, K == NULL, an image under 16 x 16, or selection_map == NULL on a frame without pyramid levels 0..2; SDSO_ERR_STATE
 * when selection_map == NULL and no sdso_pixel_select state can be made on frame_slot (an image smaller than one 32 x 32 cell).
 *
 * sdso_init_get_pnts: the Pnt members in points[0] order, one copy; null members are skipped; out->n is set.
 *
 * sdso_init_from_initializer = initializeFromInitializer STEP 3 (FullSystem.cpp:1533-1573) on the kept state.  For every Pnt i in order:
 *   keep[i] == 0: `rand()/(float)RAND_MAX > keepPercentage` held (:1535; the draws belong to the caller's process); NULL = no Pnt skipped
 *   ImmaturePoint(point->u+0.5f, point->v+0.5f, firstFrame, point->my_type, &Hcalib) (:1538: the (int u_, int v_, ...) constructor,
 *   ImmaturePoint.cpp:33, so the pixel is (x, y) again), the interval 0 / NaN, traceStereo(firstFrameRight, K, 1) (:1540-1545): the same
 *   inputs, pixel and interval as in setFirstStereo and a deterministic trace, so the device keeps the first trace's color, weights,
 *   energyTH, idepth_min_stereo, idepth_max_stereo, idepth_stereo and status per Pnt and does not trace again
 *   dropped if !isfinite(energyTH) || !isfinite(idepth_min) || !isfinite(idepth_max) || idepth_min < 0 || idepth_max < 0 (:1552-1559).
 *   Every survivor is IPS_GOOD: all other exits of traceStereo leave idepth_max_stereo NaN, except ImmaturePoint.cpp:440-443 (OUTLIER with
 *   idepth_max_stereo < 0)
 *   PointHessian(pt) copies u v my_type color[8] weights[8] energyTH (HessianBlocks.cpp:35-68; maxRelBaseline, numGoodResiduals and
 *   idepth_hessian are 0); setIdepthScaled(idepth_stereo), setIdepthZero(idepth_stereo), hasDepthPrior = true, ACTIVE (:1565-1568)
 *   counts (4 ints, may be NULL): [0] Pnts walked, [1] skipped by keep, [2] dropped by :1552-1559, [3] points made
 * Copies the flags up and the counts back; n_points == NULL and counts == NULL only enqueue.  Does not change the Pnt state: the call is
 * repeatable with other flags, and sdso_init_get_pnts returns the same bytes before and after.
 *
 * sdso_init_get_points: firstFrame->pointHessians of the latest sdso_init_from_initializer in push order, one copy; null members are
 * skipped; out->n is set.  pnt = the index into points[0]; idepth = idepth_scaled = idepth_zero; idepth_min / idepth_max are the
 * ImmaturePoint's (:1547-1548), which PointHessian does not keep.
 * SDSO_ERR_STATE: sdso_init_from_initializer / sdso_init_get_* before a sdso_init_set_first_stereo (or after sdso_init_release), and
 * sdso_init_get_points before a sdso_init_from_initializer on the current state. */
#define SDSO_INIT_NCOUNTS 8
int sdso_init_set_first_stereo(sdso_ctx* ctx, int frame_slot, int right_slot, const float K[4], float baseline,
                               const float* selection_map, int* numPoints, int* counts);
typedef struct { int n; float *u, *v, *idepth, *iR, *my_type; uint8_t* status; } sdso_init_pnts_t;
int sdso_init_get_pnts(sdso_ctx* ctx, sdso_init_pnts_t* out);
int sdso_init_from_initializer(sdso_ctx* ctx, const uint8_t* keep, int* n_points, int* counts);
typedef struct { int n; int* pnt; float *u, *v, *my_type, *idepth, *idepth_min, *idepth_max, *energyTH, *color /* n*8 */, *weights /* n*8 */; } sdso_init_points_t;
int sdso_init_get_points(sdso_ctx* ctx, sdso_init_points_t* out);
int sdso_init_release(sdso_ctx* ctx);

/* ------------------------------------------------------------------ the device-resident immature points
 * One set per ctx: the ImmaturePoint objects of every keyframe of the window (host->immaturePoints, HessianBlocks.h), grouped by a
 * caller-chosen host_id, each group in the order of the reference's vector.  Stored per point, exactly the members the reference carries
 * (ImmaturePoint.h:60-102): u, v, my_type, idepth_min, idepth_max, quality, color[8], weights[8], gradH[4], energyTH, lastTraceStatus,
 * lastTraceUV[2], lastTracePixelInterval.  The order of a host's points is part of the state (activatePointsMT STEP 2,
 * FullSystem.cpp:837-902, walks it in index order).  The set has buffers of its own: no other entry point reads or writes them.
 * A call that needs a host's count on the host side waits for the add that made it (an event, not the stream); nothing else synchronises
 * unless stated. */

/* FullSystem::makeNewTraces, the loop at FullSystem.cpp:1611-1626: for y in [3, h-4), x in [3, w-4) (patternPadding = 2) every pixel with
 * map != 0 becomes ImmaturePoint(x, y, frame, map[i]) (ImmaturePoint.cpp:33-62: idepth_min 0, idepth_max NaN, quality 10000,
 * IPS_UNINITIALIZED; lastTraceUV and lastTracePixelInterval, which the reference leaves uninitialised, are 0); a point whose energyTH is
 * not finite is dropped (:1619-1621); the survivors become the points of host_id in raster order.  Both compactions (map entries, then
 * survivors) run on the device in order.
 *   selection_map : w*h host floats, or NULL = the map of the latest sdso_pixel_select of this ctx, which must have been made on
 *                   frame_slot (SDSO_ERR_STATE otherwise)
 *   n_out         : the number of points stored; NULL = enqueue only (reading the count waits for the device)
 * SDSO_ERR_ARG for a host_id that already has points (sdso_imm_release_host first). */
int sdso_imm_add_frame(sdso_ctx* ctx, int host_id, int frame_slot, const float* selection_map, int* n_out);

/* FullSystem::traceNewCoarseKey (FullSystem.cpp:745-781, right_slot < 0) and traceNewCoarseNonKey (:632-742, right_slot >= 0) on the set,
 * in place.  geom[g] names a host and carries what the caller computes at :654-665: KRKi = K R K^-1, Kt = K t, aff =
 * AffLight::fromToVecExposure(...), KRi = K R^-1, t, all as floats; Ki is the caller's K.inverse() (:645); K = {fx,fy,cx,cy}.  Hosts of
 * the set that geom does not name are left untouched.  At most SDSO_IMM_MAX_HOSTS geometries per call.
 *   every point of every named host: ImmaturePoint::traceOn(frame_slot, KRKi, Kt, aff) (ImmaturePoint.cpp:459-828)
 *   non-key, for every point whose traceOn returned IPS_GOOD (floats, one rounding per operation, row products summed left to right):
 *     idepth_{min,max}_project = 1 / (KRKi * (Vec3f(u,v,1) / idepth_{min,max}) + Kt)[2]                                   (:675-679)
 *     fwd  = ImmaturePoint(lastTraceUV, frame_slot) with idepth_min = idepth_min_stereo = min_project, idepth_max_stereo =
 *            max_project, traced by traceStereo(right_slot, K, 1)                                                         (:672-689)
 *     back = if fwd is IPS_GOOD: ImmaturePoint(fwd.lastTraceUV, right_slot) with the projected interval, traceStereo(frame_slot, K, 0);
 *            its status is not examined                                                                                   (:691-700)
 *     if |fwd.u_stereo - back.lastTraceUV[0]| > 1 and fwd.u_stereo - fwd.lastTraceUV[0] < 10: lastTraceStatus = IPS_OUTLIER, nothing
 *     else changes; otherwise idepth_{min,max} = 1 / (KRi * (Ki * Vec3f(fwd.u_stereo, fwd.v_stereo, 1) / fwd.idepth_{min,max}_stereo
 *     - t))[2]                                                                                                            (:703-720)
 *   Both traceStereo launches use the ctx's refinement mode (sdso_trace_set_gn_mode).  A GOOD lastTraceUV outside [2, w-3) x [2, h-3),
 *   where the reference's constructor would read outside the image, takes no (further) stereo step and is counted as unreadable.
 *   counts : NULL = enqueue only.  Otherwise SDSO_IMM_NCOUNTS ints, after a synchronisation: [0..5] the histogram of lastTraceStatus over
 *            the traced points as the call leaves it, [6] forward traces that were IPS_GOOD, [7] points set IPS_OUTLIER by the stereo
 *            rule, [8] intervals updated, [9] unreadable points ([6..9] are 0 for the key form).
 * SDSO_ERR_ARG before any device work for an unknown host_id, one named twice, or a frame of another size than the host's. */
#define SDSO_IMM_MAX_HOSTS 8
#define SDSO_IMM_NCOUNTS 10
typedef struct { int host_id; float KRKi[9]; float Kt[3]; float aff[2]; float KRi[9]; float t[3]; } sdso_imm_geom_t;
int sdso_imm_trace(sdso_ctx* ctx, int frame_slot, int right_slot, int ngeom, const sdso_imm_geom_t* geom, const float K[4],
                   const float Ki[9], float baseline, int* counts);

/* FullSystem::stereoMatch, the loop at FullSystem.cpp:581-613 (the stereo-only mode, main_dso_pangolin.cpp:481-491), on the points of
 * group host_id after sdso_imm_add_frame (makeNewTraces, :577).  For every point i of the group, in group order:
 *   fwd  = the point itself — its stored u, v, colour, weights, gradH, energyTH, quality and last trace, not re-sampled from frame_slot —
 *          with u_stereo = u, v_stereo = v, idepth_min = idepth_min_stereo = 0, idepth_max_stereo = NaN whatever interval the set stores,
 *          traced by traceStereo(right_slot, K, 1)                                                                          (:582-587)
 *   back = if fwd is IPS_GOOD: ImmaturePoint(fwd.lastTraceUV, right_slot) with the interval 0 / NaN, traceStereo(frame_slot, K, 0)  (:589-596)
 *   accepted = back is IPS_GOOD and |u - back.lastTraceUV[0]| < 1 and depth > 0 and depth < max_depth, depth = 1.0f / fwd.idepth_stereo
 *          (:598-601; the reference passes 70)
 * A GOOD fwd.lastTraceUV outside [2, w-3) x [2, h-3), where the reference's constructor would read outside the image, takes no back trace,
 * is counted as unreadable and is not accepted (the rule of sdso_imm_trace).  Both traces use the ctx's refinement mode
 * (sdso_trace_set_gn_mode).  The group is NOT changed (the reference deletes the frame right after the loop): a second call returns the
 * same bytes, and sdso_imm_get what it returned before.
 *   build_map : non-zero = the dense image of :606-608 is built on the device: cleared, then every accepted point writes its three floats
 *               at pixel ((int)v, (int)u).  A group of sdso_imm_add_frame holds at most one point per pixel.  For other groups
 *               (sdso_imm_put_host) the per-point arrays are the result: a pixel claimed twice holds one of the contenders, and a point
 *               whose pixel is not in the image writes none.  The map stays on the device until the next call that builds one;
 *               sdso_imm_stereo_map_dev returns it (SDSO_ERR_STATE before the first such call).
 *   out       : caller-owned arrays for the group's n points (sdso_imm_count), every member may be NULL
 *   counts    : SDSO_IMM_MATCH_NCOUNTS ints or NULL: [0] points walked, [1] forward IPS_GOOD, [2] back traces run, [3] back IPS_GOOD,
 *               [4] accepted (the reference's `counter`), [5] back GOOD but |du| >= 1, [6] back GOOD, |du| < 1, depth outside
 *               (0, max_depth), [7] unreadable; [3] = [4] + [5] + [6]
 * out == NULL and counts == NULL: the call only enqueues.  Otherwise one copy back and one synchronisation (13 bytes per point, 15 with a
 * status array), and a second copy for out->map.  The per-point results have buffers of their own: sdso_imm_stereo_match_fetch returns
 * them until the next sdso_imm_stereo_match, whatever other sdso_imm_* calls run in between (SDSO_ERR_STATE before the first call;
 * SDSO_ERR_ARG for out->map when the latest call built no map).
 * Refused with SDSO_ERR_ARG before any device work, the set, the kept results and the kept map left as they were: an unknown host_id, an
 * unknown frame_slot or right_slot, a pyramid of another size than the group's w x h, K == NULL, a max_depth that is not > 0 (NaN
 * included), out->map without build_map.  An empty group is not an error: the counts are 0 and the map, if asked for, is all zeros. */
#define SDSO_IMM_MATCH_NCOUNTS 8
typedef struct {
  uint8_t* accepted;     /* n      1 where :601 holds                                                        */
  float*   idepth;       /* n*3    idepth_stereo, idepth_min_stereo, idepth_max_stereo of the forward trace
                                   (what :606-608 write); 0 0 0 where not accepted                           */
  uint8_t* status_fwd;   /* n      ImmaturePointStatus of :587                                               */
  uint8_t* status_back;  /* n      of :596; 255 where the back trace did not run                             */
  float*   map;          /* w*h*3  row-major, pixel ((int)v, (int)u), 3 floats as :606-608; 0 elsewhere      */
} sdso_imm_match_out_t;  /* every member may be NULL */
int sdso_imm_stereo_match(sdso_ctx* ctx, int host_id, int frame_slot, int right_slot, const float K[4], float baseline,
                          float max_depth /* the reference: 70 */, int build_map, sdso_imm_match_out_t* out /* NULL: enqueue only */,
                          int* counts /* NCOUNTS or NULL */);
/* the kept results of the latest sdso_imm_stereo_match again (what :598-608 decided and wrote), e.g. after an enqueue-only call; out->map
 * only if that call built the map */
int sdso_imm_stereo_match_fetch(sdso_ctx* ctx, sdso_imm_match_out_t* out, int* counts);
/* the idepth image of :606-608 where the latest map-building call left it: a device pointer, valid until the next such call or
 * sdso_ctx_destroy */
int sdso_imm_stereo_map_dev(sdso_ctx* ctx, void** map_dev /* float*, w*h*3 */, int* w, int* h);

/* host->immaturePoints.size() (0 for a host the set does not hold), and one host's points copied back in the traceOn convention of
 * sdso_trace_points_t: u_stereo / v_stereo = u / v, idepth_min_stereo / idepth_max_stereo = idepth_min / idepth_max; out->idepth_min and
 * out->idepth_stereo are not written; null members are skipped; out->n is set.  This is the per-keyframe download that feeds
 * sdso_activate_select and sdso_activate_points_batch.  sdso_imm_get returns SDSO_ERR_ARG for an unknown host_id. */
int sdso_imm_count(sdso_ctx* ctx, int host_id, int* n);
int sdso_imm_get(sdso_ctx* ctx, int host_id, sdso_trace_points_t* out, float* my_type);

/* FullSystem::activatePointsMT STEP 5 (FullSystem.cpp:948-957): `if entry i is flagged: entry i = back(); pop_back(); i--`, the entry moved
 * in being examined again.  Host only: src[j] (j < *n_out) is the old index of the entry that ends at index j.
 * sdso_imm_remove applies that order to a host's arrays with a gather on the device (enqueue only); n must be the host's count. */
int sdso_imm_remove_order(int n, const uint8_t* flags, int* n_out, int* src);
int sdso_imm_remove(sdso_ctx* ctx, int host_id, int n, const uint8_t* flags);
/* the points of a frame that leaves the window (`delete` of FrameHessian::immaturePoints, HessianBlocks.h); an unknown host_id is not an
 * error */
int sdso_imm_release_host(sdso_ctx* ctx, int host_id);

/* The inverse of sdso_imm_get: installs the n = pts->n points of host_id from host arrays in sdso_imm_get's convention (u_stereo /
 * v_stereo = u / v, idepth_min_stereo / idepth_max_stereo = idepth_min / idepth_max; pts->idepth_min and pts->idepth_stereo are not read)
 * plus my_type, for a host image of w x h.  For a caller that switches to the resident set in mid-run or made the points on the host.
 * n = 0 installs an empty group.  SDSO_ERR_ARG for a host_id that already has points, a null member with n > 0, or w, h < 16. */
int sdso_imm_put_host(sdso_ctx* ctx, int host_id, int w, int h, const sdso_trace_points_t* pts, const float* my_type);

/* FullSystem::activatePointsMT STEP 2-5 (FullSystem.cpp:837-957) on the set, in place, after sdso_distmap_make (STEP 1 and
 * makeDistanceMap stay with the caller).  The candidates are the points of frames 0 .. nf-2 concatenated in frame order, each group in
 * its set order; the group of the newest frame (the last one), if it has one, is neither walked nor changed.
 *   STEP 2 (:845-901)  sdso_activate_select's rules and contract per candidate: the gates, then the distance test and addIntoDistFinal in
 *                      candidate order on the ctx's map; the re-grown map is left in the ctx
 *   STEP 3 (:907-917)  every SELECTed candidate goes through optimizeImmaturePoint (FullSystemOptPoint.cpp:52-238) against the other
 *                      nf-1 frames at pyramid level 0: the status, currentIdepth and ResStates of sdso_activate_points_batch
 *   STEP 4 (:919-945)  an entry leaves the set if STEP 2 decided DELETE, or it was selected and its status is 1 or -1, or it was
 *                      selected with status 0 and its lastTraceStatus is IPS_OOB; a selected entry with status 0 that is not OOB stays
 *   STEP 5 (:948-957)  every walked group is compacted in the order sdso_imm_remove_order defines, computed on the device
 * One enqueue of the whole chain, one copy of the results back and one synchronisation (a second copy only past
 * SDSO_IMM_ACT_FIRST_COPY selected points).
 *   host_id[f]      : the group of frame f in the set; a frame without a group has no candidates (not an error)
 *   frame_slot[f]   : pyramid slots, level 0 is read
 *   host_flagged[f] : FrameHessian::flaggedForMarginalization
 *   geom[f]         : KRKi / Kt of frame f into the newest (:841-842), f < nf-1
 *   pair_R/t/aff    : host->targetPrecalc[target->idx] PRE_RTll / PRE_tTll / PRE_aff_mode, indexed host*nf+target, as in sdso_activate_t
 *   minObs          : the reference passes 1 (FullSystem.cpp:790)
 *   counts          : SDSO_IMM_ACT_NCOUNTS ints (may be NULL): [0] candidates, [1..3] STEP 2 decisions KEEP / DELETE / SELECT,
 *                     [4] toOptimize.size(), [5..7] statuses -1 / 0 / 1, [8] entries removed in STEP 4, [9 + f] the new count of frame
 *                     f's group (0 without a group, unused entries 0)
 * Refused before any device work, the set and the map left as they were: SDSO_ERR_STATE without a map; SDSO_ERR_ARG for nf outside
 * 2..8, a host_id named twice, an unknown frame_slot, a pyramid or a group of another size than w x h, w>>1, h>>1 other than the map's. */
#define SDSO_IMM_ACT_NCOUNTS 17
#define SDSO_IMM_ACT_FIRST_COPY 1024
typedef struct {
  int nf;                            /* frames of the window in frameHessians order, 2..8; the last one is the newest */
  const int* host_id;
  const int* frame_slot;
  const uint8_t* host_flagged;
  const sdso_distmap_geom_t* geom;   /* nf-1 */
  const float* pair_R; const float* pair_t; const float* pair_aff;   /* nf*nf */
  int w, h;
  float K[4];                        /* fxl fyl cxl cyl */
  int minObs;
  float currentMinActDist;           /* after STEP 1 (:798-817) */
  float minTraceQuality;             /* setting_minTraceQuality = 3 (settings.cpp:112) */
} sdso_imm_activate_t;
int sdso_imm_activate(sdso_ctx* ctx, const sdso_imm_activate_t* A, int* counts);

/* The results of the latest sdso_imm_activate of this ctx, kept by the library until the next one (SDSO_ERR_STATE before the first).
 * The records are also kept on the device, in a buffer of the set that no other call writes, with the w x h of the call and a
 * "consumed" flag that every sdso_imm_activate clears: sdso_ba_window_update_activated reads them there.
 * One entry per selected candidate in toOptimize order, n = counts[4]; arrays are caller-owned, null members are skipped, out->n and
 * out->nf are set.
 *   frame, index : the candidate's frame and idxInImmaturePoints, its index in the group BEFORE the removal
 *   status, idepth, res_state[n * nf] : as sdso_activate_points_batch (255 for the host itself / not evaluated)
 *   u .. weights : the members PointHessian::PointHessian(const ImmaturePoint*, ...) copies (HessianBlocks.cpp:35-70)
 *   decision     : the STEP 2 decision of every candidate (counts[0] bytes: 0 KEEP, 1 DELETE, 2 SELECT), may be NULL */
typedef struct {
  int n, nf;
  int* frame; int* index;
  int8_t* status; float* idepth; uint8_t* res_state;
  float* u; float* v; float* my_type; float* idepth_min; float* idepth_max; float* energyTH;
  float* color;      /* n*8 */
  float* weights;    /* n*8 */
  uint8_t* lastTraceStatus;
} sdso_imm_activated_t;
int sdso_imm_activate_fetch(sdso_ctx* ctx, sdso_imm_activated_t* out, uint8_t* decision);

/* ------------------------------------------------------------------ the fork's live g2o factors
 * gyubeomim/stereo-dso-g2o routes tracking, window optimisation and the sub-pixel trace refinement through g2o edges
 * (src/FullSystem/dso_g2o_edge.cpp, dso_g2o_vertex.cpp).  The edges' own arithmetic is specified by the reference tree and
 * is reproduced here exactly; g2o itself (robust kernel, quadratic form, Levenberg-Marquardt / Gauss-Newton control) is
 * neither vendored nor version-pinned (CMakeLists.txt:47-58) and is restated from its published algorithm — "parity
 * unpinned" for everything g2o decides.  `SE3 * Vec3` is evaluated as R*X + t with R = rotationMatrix(). */

/* S3: sub-pixel refinement used by every later traceStereo launch of this ctx (sdso_trace_stereo_*, sdso_stereo_match_batch):
 *   0  DSO-native GN, ImmaturePoint.cpp:707-769 (default)
 *   1  fork-live: VertexUVDSO + 8 EdgeTracePointUVDSO (dso_g2o_edge.cpp:571-619, dso_g2o_vertex.cpp:65-88), Huber(9),
 *      one g2o Gauss-Newton iteration per pass, 3 passes (ImmaturePoint.cpp:309-412) */
int sdso_trace_set_gn_mode(sdso_ctx* ctx, int mode);

/* T5: EdgeSE3PosePhotoDSO (dso_g2o_edge.cpp:395-500) at one evaluation point. */
typedef struct {
  int lvl, w, h;
  float fx, fy, cx, cy;      /* KG[level] (Matrix3f, globalCalib.cpp:90-107) = CoarseTracker fx[lvl]..cy[lvl] */
  float Ki[9];               /* Ki[lvl]                                              CoarseTracker.cpp:130  */
  float RKi[9], t_cull[3];   /* calcRes :617-618 from the pose calcRes is CALLED with (the fork always passes the
                                initial lastToNew_out, :890) — used for the border cull and the flow indicators only */
  double R[9], t[3];         /* VertexSE3PoseDSO::estimate(): rotationMatrix(), translation() */
  float ab[2];               /* AffLight::fromToVecExposure(ref_exposure, new_exposure, a0b0, VertexPhotometricDSO::estimate()).cast<float>() */
  double b0;                 /* a0b0_.b = lastRef_aff_g2l.b */
  float cutoffTH, huberTH;   /* setting_coarseCutoffTH (edges with error > 10*cutoffTH are dropped, :724), setting_huberTH */
} sdso_g2o_track_eval_t;
/* CoarseTracker::calcRes, fork-live body (CoarseTracker.cpp:600-792) for level ev->lvl of reference `ref_slot` against frame
 * `frame_slot`: culls the pc points, creates the edges, evaluates them at the vertices' estimates and keeps those that are
 * not saturated.  The edge set {mask, Xref, measurement} stays on the device, keyed by (ref_slot, level).
 *   res6     : the Vec6 calcRes returns (:783-789; E is never accumulated by the live body -> 0)
 *   n_edges  : numTermsInE;  edge_mask[pc_n], Xref[3*pc_n] optional copies (tests) */
int sdso_g2o_track_add_edges(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_g2o_track_eval_t* ev, double* res6,
                             int* n_edges, uint8_t* edge_mask, float* Xref);
/* computeActiveErrors + linearizeOplus + g2o's robustified quadratic form over that edge set at the vertex estimates in ev:
 *   H[64] row-major over [pose 6 | photometric 2], b[8], chi2 = {sum e^2, sum rho0 (activeRobustChi2)};
 *   err[pc_n], J[8*pc_n] optional per-edge values (0 where the point carries no edge). */
int sdso_g2o_track_linearize(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_g2o_track_eval_t* ev, double* H, double* b,
                             double* chi2, double* err, double* J);
/* CoarseTracker::trackNewestCoarse as the fork runs it (CoarseTracker.cpp:827-1069): per level add_edges, then g2o's
 * Levenberg-Marquardt (lambda0 0.01, 2 iterations, gain threshold 1e-3) on the 8-parameter system.  Same in/out convention
 * as sdso_track_newest_coarse; prm->maxIterations is ignored (the fork hard-codes {2,2,2,2,2}, :861). */
int sdso_g2o_track_newest_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm,
                                 sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l, sdso_track_result_t* out);
/* The same for `nhyp` independent (reference, frame, initial pose) tries, device-resident: ONE launch, one workgroup per try, every
 * calcRes, linearisation and Levenberg-Marquardt decision of CoarseTracker.cpp:827-1069 inside it (the single call above pays a launch
 * and a stream wait per evaluation and stays as the A/B).  Same shape and in/out convention as sdso_track_newest_coarse_batch;
 * prms[k].maxIterations is ignored (:861).  A try that aborts (:1032) leaves its lastToNew / aff_g2l entries untouched; one that reaches
 * :1044-1045 has written them, whatever STEP4 (:1050-1068) then returns — as the single call.  A try's numbers do not depend on nhyp or on
 * its place in the batch, and a repeated call gives the same bytes; they agree with the single call's to the order of its sums (not bit for
 * bit), the flow indicators bit for bit.  The edge sets of sdso_g2o_track_add_edges are neither read nor written.  "Parity unpinned" for
 * everything g2o decides, as above.
 * Refusals (SDSO_ERR_ARG, before any device work, nothing written): a null argument, nhyp < 1, coarsestLvl out of range, an unknown slot,
 * a frame without a level the try walks, a level size other than the uploaded one. */
int sdso_g2o_track_newest_coarse_batch(sdso_ctx* ctx, int nhyp, const int* ref_slots, const int* frame_slots,
                                       const sdso_track_params_t* prms, sdso_se3_t* lastToNew, sdso_aff_t* aff_g2l,
                                       sdso_track_result_t* outs);
/* FullSystem::trackNewCoarse STEP2-4 (FullSystem.cpp:436-511) with the fork-live trackNewestCoarse inside the loop: sdso_track_new_coarse
 * with the runner swapped — its signature, its records (sdso_track_try_t), its refusals and its two phases.  Phase 1 is try 0 alone (a
 * batch of one under NaN bounds), then the loop's rules; where the loop stops there the call returns.  Phase 2 runs tries 1..ntries-1 in
 * ONE launch of sdso_g2o_track_newest_coarse_batch under achievedRes as try 0 left it, and the rules walk the event traces in list order.
 * The fork-live body never repeats a level (levelCutoffRepeat stays 1, CoarseTracker.cpp:891-904): a trace has at most five events, and a
 * try's evaluations do not depend on minResForAbort until the test of :1032 fires, so the two facts above sdso_track_trace_t hold as they
 * stand.  Tries after the stop are reported with ran = 0.  prm->minResForAbort and prm->maxIterations are ignored. */
int sdso_g2o_track_new_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries,
                              const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold,
                              sdso_track_tries_result_t* out, sdso_track_try_t* recs);

/* B13: EdgeLBASE3PosePhotoIdepthCamDSO (dso_g2o_edge.cpp:5-282) for the nr active residuals of a window, laid out as
 * FullSystem::optimize builds the graph (FullSystemOptimize.cpp:455-542): one pose + one photometric vertex per HOST frame,
 * one idepth vertex per RESIDUAL, one camera vertex; the target pose is a constant (PRE_worldToCam). */
typedef struct {
  int nf, nr, w, h;
  const int* frame_slot;         /* nf level-0 images */
  const float* const* dI;        /* unused by the library (kept so that the layout equals the test oracle's) */
  const float* pair_R;           /* [host*nf+target] 9: (Ttw * Twh).rotationMatrix().cast<float>()   :27-30 */
  const float* pair_t;           /* [host*nf+target] 3: translation */
  const float* pair_ab;          /* [host*nf+target] 2: fromToVecExposure(host, target, a0b0 = host vertex, a1b1 = target aff).cast<float>() :85-91 */
  const double* host_b0;         /* nf: b0_ (SetB, FullSystemOptimize.cpp:527-528) */
  const float* frameEnergyTH;    /* nf */
  double cam[4];                 /* VertexCamDSO::estimate(): fx fy cx cy */
  const int* host; const int* target;        /* nr */
  const float* u; const float* v;            /* nr: r->point->u, v */
  const double* idepth;          /* nr: VertexInverseDepthDSO::estimate() */
  const float* color; const float* weights;  /* nr*8: r->point->color (= measurement), weights */
} sdso_g2o_lba_t;
/* computeError + linearizeOplus for every residual:
 *   error[nr*8] (double), J[nr*8*13] rows = [xi 6 | photometric 2 | idepth 1 | camera 4] (zero where linearizeOplus returns early),
 *   state[nr] (0 IN, 1 OOB, 2 OUTLIER), energy[nr*2] = {state_NewEnergy, state_NewEnergyWithOutlier},
 *   centerProjectedTo[nr*3] ((2,2,0) if the centre pixel was not reached), idepth_hessian[nr], edge_level[nr] (1 = setLevel(1), :60-65) */
int sdso_g2o_lba_eval(sdso_ctx* ctx, const sdso_g2o_lba_t* L, double* error, double* J, uint8_t* state, float* energy,
                      float* centerProjectedTo, float* idepth_hessian, uint8_t* edge_level);

/* FullSystem::optimize as the fork compiles it (FullSystemOptimize.cpp:402-868): g2o's Levenberg-Marquardt with a Schur block solver
 * over the graph of :455-542, every evaluation, linearisation, Schur complement and back-substitution on the device.  The caller
 * flattens its graph into arrays as for sdso_g2o_lba_eval; g2o's graph plumbing is not rebuilt.  Everything g2o decides is restated
 * from its published algorithm ("parity unpinned", above): the call is held to tests/g2o_lba_ref.py, the same algorithm in NumPy.
 *
 * W, the graph as :455-542 builds it (constant over the call): */
typedef struct {
  int nf, nr, w, h;              /* nf 1..8 frames, nr residuals (edges) in any order; the fork's is host-major (:441-453) */
  const int* frame_slot;         /* nf level-0 images */
  const sdso_se3_t* Ttw;         /* nf: r->target->PRE_worldToCam, read by the edge as a constant          dso_g2o_edge.cpp:23 */
  const sdso_aff_t* target_aff;  /* nf: r->target->aff_g2l()                                               dso_g2o_edge.cpp:87 */
  const float* ab_exposure;      /* nf: FrameHessian::ab_exposure                                          dso_g2o_edge.cpp:88-89 */
  const double* host_b0;         /* nf: b0_ (SetB at graph build, never refreshed)                         FullSystemOptimize.cpp:535-536 */
  const float* frameEnergyTH;    /* nf                                                                     dso_g2o_edge.cpp:119 */
  const int* host; const int* target;        /* nr: r->host->idx, r->target->idx                           FullSystemOptimize.cpp:478-522 */
  const float* u; const float* v;            /* nr: r->point->u, v                                         dso_g2o_edge.cpp:36-37 */
  const float* color; const float* weights;  /* nr*8: the measurement (:524-527) and r->point->weights (dso_g2o_edge.cpp:107) */
} sdso_g2o_lba_window_t;
/* S, the vertex estimates: read at entry, written at exit (a refused or failed call writes nothing). */
typedef struct {
  sdso_se3_t* Twh;               /* nf: VertexSE3PoseDSO = r->host->PRE_camToWorld      FullSystemOptimize.cpp:485 */
  sdso_aff_t* host_aff;          /* nf: VertexPhotometricDSO = r->host->aff_g2l()       :490-494 */
  double cam[4];                 /* VertexCamDSO: fxl fyl cxl cyl                       :457-458 */
  double* idepth;                /* nr: VertexInverseDepthDSO, one per RESIDUAL         :506-512 */
} sdso_g2o_lba_state_t;
typedef struct {
  int max_iterations;            /* optimize(mnumOptIts): the caller applies the 10 / 7 / 3 rule of :406-418 */
  double lambda_init;            /* setUserLambdaInit(0.1)                              :426 */
  double gain_threshold;         /* terminateAction->setGainThreshold(1e-3)             :432 */
  int max_trials;                /* g2o's maxTrialsAfterFailure default, 10 */
} sdso_g2o_lba_opt_t;
#define SDSO_G2O_LBA_MAX_RECORDED 64
#define SDSO_G2O_LBA_STOP_ITERATIONS 0  /* the iteration cap */
#define SDSO_G2O_LBA_STOP_GAIN 1        /* 0 <= (lastChi - chi) / chi < gain_threshold after an iteration */
#define SDSO_G2O_LBA_STOP_TRIALS 2      /* max_trials trials in one iteration */
#define SDSO_G2O_LBA_STOP_RHO_ZERO 3    /* a trial with rho == 0 */
#define SDSO_G2O_LBA_STOP_LAMBDA 4      /* lambda no longer finite */
typedef struct {
  int iterations, stop, n_active;           /* iterations run, SDSO_G2O_LBA_STOP_*, edges with level 0 after the build-time computeError (:539) */
  int trials[SDSO_G2O_LBA_MAX_RECORDED];    /* per iteration (the first 64 are recorded): trials, ...                          */
  double lambda[SDSO_G2O_LBA_MAX_RECORDED]; /* ... lambda after it, ...                                                          */
  double chi2[SDSO_G2O_LBA_MAX_RECORDED];   /* ... activeRobustChi2 of the terminate action's computeActiveErrors after it      */
  double chi2_final;                        /* activeRobustChi2 at the returned estimates */
  float rmse;                               /* :867: sqrtf(chi2 / (8 * nr)), nr = all edges as optimizer->edges().size(); 0 for nr = 0 */
  /* per residual, caller-owned, from the evaluation at the returned estimates (the terminate action's is the last to run): */
  uint8_t* state;                /* nr: state_NewState, sdso_g2o_lba_eval's convention */
  float* energy;                 /* nr*2: state_NewEnergy, state_NewEnergyWithOutlier */
  float* centerProjectedTo;      /* nr*3                                                                    :723 */
  uint8_t* edge_level;           /* nr: 1 if ANY computeError of the call ran setLevel(1) on the edge (dso_g2o_edge.cpp:63: never lowered) */
  float* idepth_hessian;         /* nr: of the LAST linearizeOplus = the start of the last iteration, what :726 reads; 0 where that one
                                    returned early, for an inactive edge, and after zero iterations */
  uint8_t* active;               /* nr: the edge is in g2o's active set (level 0 at initializeOptimization, :587) */
} sdso_g2o_lba_result_t;
/* The rules.
 *   pair tables : R, t = (Ttw[t] * Twh[h]) rotation and translation cast to float (dso_g2o_edge.cpp:25-28); ab = fromToVecExposure(
 *                 ab_exposure[h], ab_exposure[t], host_aff[h], target_aff[t]) cast to float (:91).  Formed on the host in double from the
 *                 estimates before every evaluation.
 *   active set  : fixed by the first evaluation (edge_level == 0 there); an inactive edge keeps its idepth, a host without an active
 *                 edge keeps its pose and affine pair.  The Jacobian of an edge is zero wherever linearizeOplus returns early
 *                 (level 1, OOB, non-finite sample: dso_g2o_edge.cpp:131, :183, :194, :204); its error is what computeError gives.
 *   kernel      : g2o's Huber on the squared norm of the 8-vector, delta = setting_huberTH (FullSystemOptimize.cpp:529-531);
 *                 H += J^T rho1 J, b -= rho1 J^T e.
 *   LM          : csrc/g2o_lm.h.  lambda is added to every diagonal, the idepth ones included, BEFORE the Schur complement, and
 *                 computeScale runs over the whole solution, idepth increments included: g2o's block solver does both.
 *   updates     : exp(d) * Twh, a += d, b += d, idepth += d, cam += d (dso_g2o_vertex.cpp:15-18, :30-40, :56-58, :100-106).
 *   sums        : every cross-edge sum is f64 over per-workgroup partials folded in a fixed order, no floating-point atomics: two calls
 *                 on the same inputs agree bit for bit.
 *   traffic     : the residual arrays go up once and the per-residual results come down once; per linearisation 8 x 91 doubles come
 *                 down, per trial 8 x 91 + 2 doubles come down and the pair tables (<= 64 x 14 floats) and the 68 increments go up.
 * SDSO_ERR_ARG with a message, nothing written: a null argument or array, nf outside 1..8, nr < 0, an unknown slot or one of another
 * size than w x h, host / target out of range, a non-finite pose, affine pair, exposure, camera value, u, v or idepth,
 * max_iterations < 0, max_trials < 1.  nr == 0 or no active edge: SDSO_OK, zero iterations, estimates untouched. */
int sdso_g2o_lba_optimize(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, sdso_g2o_lba_state_t* S,
                          sdso_g2o_lba_result_t* out);

/* The same optimiser with the Levenberg-Marquardt loop resident on the device, enqueue-only: the same W, P and S, "The rules." above and
 * the same outputs, except that nothing comes down or goes up between the evaluations — the controller (csrc/g2o_lba_core.h), the
 * block-arrow solve, the updates and the float pair tables of the tentative estimates are a single-workgroup step on the device between
 * the wide kernels, in the operation order the host has in sdso_g2o_lba_optimize.  Between _enqueue and _fetch the host does not wait,
 * does not copy and decides nothing.  sdso_g2o_lba_optimize keeps its body and is the A/B.
 *
 * _enqueue : validates (the refusals of sdso_g2o_lba_optimize, in its words, each before any device work and leaving no job behind),
 *            sorts host-major, copies EVERY input into buffers the job owns and enqueues the whole run on the ctx's stream.  On return the
 *            caller may overwrite or free everything W, P and S0 point to.  THE FRAMES' PYRAMID SLOTS ARE NOT COPIED: the caller keeps
 *            the slots of W->frame_slot uploaded and unchanged until the fetch.  nr == 0: SDSO_OK, an empty job.
 *            One job per ctx: a second _enqueue (or _resident) before the fetch is SDSO_ERR_STATE and leaves the pending job intact.
 *            Any other call on the ctx between enqueue and fetch leaves the job's results alone (its buffers are its own);
 *            sdso_ctx_destroy with a job pending drains the stream and frees it.
 * _done    : 1 the job has finished, 0 it is still running, SDSO_ERR_STATE there is no job.  Never waits.
 * _fetch   : waits for the job and writes S and out in the caller's order under the rules above (estimates untouched after zero
 *            iterations, a host without an active edge keeps its inputs, an inactive edge its idepth).  S's and out's arrays have the
 *            sizes the job was enqueued with.  Without a job, or a second time: SDSO_ERR_STATE, nothing written.  A null argument or
 *            array: SDSO_ERR_ARG, nothing written, the job stays pending.
 * _resident: _enqueue + _fetch; S is read at entry and written at exit as in sdso_g2o_lba_optimize, whose refusals it has. */
int sdso_g2o_lba_optimize_enqueue(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, const sdso_g2o_lba_state_t* S0);
int sdso_g2o_lba_optimize_done(sdso_ctx* ctx);
int sdso_g2o_lba_optimize_fetch(sdso_ctx* ctx, sdso_g2o_lba_state_t* S, sdso_g2o_lba_result_t* out);
int sdso_g2o_lba_optimize_resident(sdso_ctx* ctx, const sdso_g2o_lba_window_t* W, const sdso_g2o_lba_opt_t* P, sdso_g2o_lba_state_t* S,
                                   sdso_g2o_lba_result_t* out);

/* ------------------------------------------------------------------ the device-resident map
 * What FullSystem::makeKeyFrame publishes through publishKeyframes (FullSystem.cpp:1467 for the whole window, FullSystemMarginalize.cpp:184
 * for a frame that leaves) and the one consumer the reference ships, KeyFrameDisplay::setFromKF / refreshPC
 * (IOWrapper/Pangolin/KeyFrameDisplay.cpp:85-165, :174-323): the points of every keyframe as 3-D vertices and colours.
 *
 * The map is one per ctx.  Keyframes are keyed by FrameHessian::frameID; each holds three growable device lists of records — pointHessians
 * (list 1), pointHessiansMarginalized (2), pointHessiansOut (3); the list is the record's status (:129, :144, :158), the immature points
 * (status 0, :104-117) are read from the resident immature set.  A record is 16 floats (csrc/map_cloud.h states it and every rule below):
 *   u, v, idepth, idepth_hessian, maxRelBaseline, color[8], 3 floats of padding (0 when the device wrote the record)
 *
 * sdso_map_update — setFromKF's copy, made while the window's post-state is valid.  For every frame of the window the keyframe's active
 * list is REPLACED by the named points in the given order; the leaving points are APPENDED to their host keyframe's marginalised or out
 * list in the given order.  A keyframe is created by the first update that names it.  Values come from the resident window (u, v, idepth;
 * maxRelBaseline and idepth_hessian of the closing linearizeAll / the last solve; the colours): only the 4-byte indices cross the bus.
 * The host supplies the orders because removeOutliers and flagPointsForRemoval walk fh->pointHessians with swap-with-back compaction,
 * which the caller's pointer graph already runs; the window's own order differs (see point_order of sdso_track_make_ref_from_window).
 *   valid when : as for sdso_ba_flag_points — an optimize call has ended on the window, no sdso_ba_window_update has run since, it holds
 *                no linearised residual (so: before sdso_ba_marginalize_points) and is outside a batch.  Otherwise SDSO_ERR_STATE.
 *   refusals   : SDSO_ERR_ARG before any device work: an unknown window, a NULL struct, an index out of range or named twice across
 *                active and gone, a gone_list byte other than 2 or 3, n_active + n_gone != np when active is given.  A refused call
 *                leaves the map as it was, and so does one that fails in its device phase (SDSO_ERR_HIP): room is made first, the
 *                new sizes are committed once the gather is enqueued.  The call changes nothing in the window.
 *   cost       : one upload of the index lists, one kernel, no read-back: enqueue only.  A list that has to grow is allocated anew
 *                (doubling) and copied device to device, which synchronises once. */
typedef struct {
  int n_active; const int* active;     /* window point indices: fh->pointHessians after FullSystem.cpp:1044-1053, frame by frame.
                                          NULL: every point not named in `gone`, in window order */
  int n_gone;   const int* gone;       /* window point indices in the order the reference pushed them this keyframe:
                                          removeOutliers' (FullSystemOptimize.cpp:1073-1079) before flagPointsForRemoval's (:997-1041) */
  const uint8_t* gone_list;            /* n_gone: 2 = pointHessiansMarginalized, 3 = pointHessiansOut */
} sdso_map_update_t;
int sdso_map_update(sdso_ctx* ctx, int win, const sdso_map_update_t* upd);
/* list sizes of a keyframe: active, marginalised, out.  SDSO_ERR_ARG for an unknown frameID (as in every call below that names one) */
int sdso_map_counts(sdso_ctx* ctx, int frameID, int* counts /* 3 */);
/* tests / debugging: list 1, 2 or 3 of a keyframe as records (counts[list - 1] * 16 floats) */
int sdso_map_get(sdso_ctx* ctx, int frameID, int list, float* records);
/* the inverse of sdso_map_get, as sdso_imm_put_host is of sdso_imm_get: REPLACES the list by n host records (a caller that joins in
 * mid-run, and the tests); creates the keyframe where it is unknown */
int sdso_map_put(sdso_ctx* ctx, int frameID, int list, int n, const float* records);
/* forget a keyframe (after its `final = true` publication) / every keyframe.  sdso_ctx_destroy frees everything. */
int sdso_map_release_keyframe(sdso_ctx* ctx, int frameID);
int sdso_map_clear(sdso_ctx* ctx);

/* refreshPC (:174-295) for up to 8 keyframes in one call.
 *   order      : frames in the given order; per frame immature, active, marginalised, out (:104-160), each in list order; per kept point
 *                its 8 vertices in patternP order.  The output is packed: first[k] is the first vertex of frame k, first[n_frames] the
 *                total.  kept[4k + s]: the POINTS of frame k with status s that passed (8 vertices each).
 *   keep tests : :215-234 in the reference's order and arithmetic (var = (float)(1.0f / ((double)idepth_hessian + 0.01))); every
 *                comparison as written, so a NaN passes — an immature point whose idepth_max is still NaN is emitted, with NaN vertices,
 *                wherever minBS <= 0 and the mode shows status 0.  Modes above 2 show nothing.
 *   vertex     : ((u + dx) * fxi + cxi) * depth, the y analogue, z = depth; float, one rounding per operation; fxi = 1/fx, cxi = -cx/fx
 *                in float (setFromF, :77-80).  camToWorld == NULL: camera-frame vertices, the buffer the reference uploads.  Otherwise
 *                X = R[0]*x + R[1]*y + R[2]*z + t[0] (rows 1, 2 alike), float, summed left to right: what Pangolin leaves to the GL matrix.
 *   colour     : mode 0 the fixed colours of :250-282, otherwise the grey triple (unsigned char)color[pnt]
 *   deviations : (1) refreshPC draws rand() for a z jitter of relative size +-fxi (:246) and for sparsity > 1 (:240), from the
 *                process-wide generator in emission order; a library cannot reproduce either.  Here z = depth — the reference's
 *                expression with every draw at 0.5 — and there is no sparsification.  (2) With no vertex the reference returns before
 *                touching its buffers; here first[] is all zeros and the arrays are untouched.  (3) The colour byte is truncation for
 *                0 <= c < 256; outside it is the low byte of x86's float -> int conversion, 0 for a NaN or a value beyond int.
 *   refusals   : SDSO_ERR_ARG before anything is launched or copied: n_frames outside 1..8, a NaN threshold, a frame named twice, an
 *                unknown frameID — these first, without touching the device —, then an unknown immature group and cap below the
 *                upper bound 8 x the sum of the list sizes (sdso_map_counts, sdso_imm_count), decided on the bound, not on the
 *                outcome.  The bound needs the groups' counts: a group whose sdso_imm_add_frame has not reported its count yet is
 *                waited for here (that add's event, as sdso_imm_count waits; not the stream).
 *   cost       : one upload of the query, two kernels, and two waits (measured equal to one wait on a copy of the upper bound,
 *                profiles/map_cloud_timing.txt): for the 128 bytes of per-list counts, which size the copy, and
 *                for the copy of the used prefix of the two arrays.  Integer counting only: a second call returns the same bytes. */
typedef struct {
  int n_frames; const int* frameID; const int* imm_host_id;   /* imm_host_id[k] < 0 or NULL: no immature list; else the sdso_imm_* group */
  float fx, fy, cx, cy;                                       /* HCalib->fxl() .. cyl() */
  float scaledTH, absTH, minBS; int mode;                     /* Pangolin's defaults: 0.001, 0.001, 0.1, 1 */
  const float* camToWorld;                                    /* n_frames*12 (R row-major, t) or NULL */
  int cap;                                                    /* vertices the caller's arrays hold */
} sdso_map_cloud_t;
int sdso_map_cloud(sdso_ctx* ctx, const sdso_map_cloud_t* q, float* xyz /* cap*3 */, uint8_t* rgb /* cap*3 */,
                   int* first /* n_frames+1 */, int* kept /* n_frames*4 per status, or NULL */);
/* the latest call's device buffers (float xyz[n*3], uint8_t rgb[n*3]) for a renderer, valid until the next sdso_map_cloud;
 * SDSO_ERR_STATE before the first */
int sdso_map_cloud_dev(sdso_ctx* ctx, void** xyz_dev, void** rgb_dev, int* n);

#ifdef __cplusplus
}
#endif
#endif /* SDSO_ABI_H */
