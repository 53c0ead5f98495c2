// The LM state machine of trackNewestCoarse, one text for the host driver and for k_track_lm (part of tracker.hip, after tracker_eval.hip: TrackOut).
// ------------------------------------------------------------------ trackNewestCoarse
// CoarseTracker::trackNewestCoarse (CoarseTracker.cpp:827-1069, DSO-native LM :908-1024) is a chain of calcRes+calcGSSSE
// evaluations with a little 8x8 algebra in between: LmCore is that state machine, written once for host and device.  It always
// has exactly one evaluation pending (first evaluation of a level, repeat with a doubled cutoff, or the trial step of an LM
// iteration).  Two drivers:
//   * k_track_lm (default): ONE launch runs the whole call — a cluster of up to eight 512-thread workgroups per motion hypothesis
//     (FullSystem::trackNewCoarse tries up to 53 of them, FullSystem.cpp:305-441; the clusters run side by side), all threads evaluate the
//     pending calcRes+calcGSSSE over the level's points, the members exchange their partial sums once, and every member solves the 8x8
//     system on one wave, applies SE3::exp and takes the accept / reject and level decisions on the same sums (see the cluster notes at
//     the kernel).  No host round trip per evaluation (it cost 25 us of launch + synchronisation each, 28 times per call).
//   * the lock-step host loop (SDSO_TRK_HOST_LM=1): every round evaluates the pending requests of all hypotheses in one k_track_eval
//     launch.  Same LmCore, same sequence of evaluations.
namespace sdso {
// ---- LM arithmetic with two callers: LmCore (the host driver; lane 0 of the device driver) and lm_wave_step (tracker_lm.hip: all lanes of
// a wave on the same numbers).  Plain values and arrays in and out — no references into LDS — so that the wave form keeps its loads together.
constexpr float kLambdaExtrapolationLimit = 0.001f;
// :966-981 — the step is stretched below the lambda limit (inc keeps the stretched step: the convergence test reads it), then scaled into
// the tangent; a non-finite sum becomes a zero step
SDSO_HD inline void lm_scale_step(float lambda, double* inc, double* incScaled) {
  float extrapFac = 1;
  if (lambda < kLambdaExtrapolationLimit) extrapFac = sqrtf(sqrtf(kLambdaExtrapolationLimit / lambda));
  for (int i = 0; i < 8; i++) { inc[i] *= extrapFac; incScaled[i] = inc[i]; }
  for (int i = 0; i < 3; i++) incScaled[i] *= SCALE_XI_ROT;
  for (int i = 3; i < 6; i++) incScaled[i] *= SCALE_XI_TRANS;
  incScaled[6] *= SCALE_A;
  incScaled[7] *= SCALE_B;
  double sum = 0;
  for (int i = 0; i < 8; i++) sum += incScaled[i];
  if (!std::isfinite(sum)) for (int i = 0; i < 8; i++) incScaled[i] = 0;
}
// :937-964 — where the solution x of the reduced system lands in inc when an affine parameter is fixed: 6 unknowns (a and b fixed), 7
// with b fixed, or 7 with a fixed (rows / columns 6 <- 7 of the system: the seventh unknown is b)
SDSO_HD inline void lm_place_reduced(bool fixA, bool fixB, const double* x, double* inc) {
  for (int i = 0; i < 6; i++) inc[i] = x[i];
  inc[6] = (fixB && !fixA) ? x[6] : 0;
  inc[7] = (fixA && !fixB) ? x[6] : 0;
}

struct LmCore {
  sdso_track_params_t p;
  sdso_track_result_t out;
  Se3 cur, Tnew;
  sdso_aff_t affCur, affNew;
  sdso_se3_t T_final; sdso_aff_t aff_final;     // what lastToNew / aff_g2l receive (only when the call reaches its end)
  bool wrote_final, haveRepeated, done;
  int lvl, iteration, phase;                    // phase 0: first / repeated evaluation of a level, 1: trial step
  float levelCutoffRepeat, lambda;
  double oldres[6];                             // calcRes' Vec6 of the accepted state
  double H[64], b[8], inc[8];
  Se3 reqT; sdso_aff_t reqAff;                  // the evaluation this hypothesis waits for
  double wHl[64], wHs[64], wnb[8], wbs[8], wx[8], wwork[80];   // work space of solve_inc() (members: in LDS on the device)
  int wperm[8];
  sdso_track_trace_t trace;                     // every finish_level event in order (at most six: five levels and one repetition) — what
                                                // sdso_track_new_coarse replays the abort test of :1032 from (track_tries.h)

  SDSO_HD void init(const sdso_track_params_t& prm, const sdso_se3_t& T0, const sdso_aff_t& aff0) {
    p = prm;
    track_result_reset(out);
    cur = se3_from_abi(T0);
    affCur = aff0;
    T_final = T0; aff_final = aff0; wrote_final = false;
    haveRepeated = false; done = false;
    trace.n = 0;
    iteration = 0; lambda = 0.01f;
    lvl = p.coarsestLvl;
    for (int i = 0; i < 8; i++) inc[i] = 0;
    for (int i = 0; i < 6; i++) oldres[i] = 0;
    start_level();
  }
  SDSO_HD void request(const Se3& T, const sdso_aff_t& a) { reqT = T; reqAff = a; }
  SDSO_HD void start_level() { levelCutoffRepeat = 1; phase = 0; request(cur, affCur); }
  SDSO_HD void finish() {   // :1044-1068
    done = true;
    wrote_final = true;
    se3_to_abi(cur, T_final);
    aff_final = affCur;
    if ((p.affineOptModeA != 0 && (fabsf((float)aff_final.a) > 1.2)) || (p.affineOptModeB != 0 && (fabsf((float)aff_final.b) > 200))) return;
    double rel[2];
    affFromTo(p.ref_exposure, p.new_exposure, p.ref_aff_g2l.a, p.ref_aff_g2l.b, aff_final.a, aff_final.b, rel);
    const float r0 = (float)rel[0], r1 = (float)rel[1];
    if ((p.affineOptModeA == 0 && (fabsf(logf(r0)) > 1.5)) || (p.affineOptModeB == 0 && (fabsf(r1) > 200))) return;
    if (p.affineOptModeA < 0) aff_final.a = 0;
    if (p.affineOptModeB < 0) aff_final.b = 0;
    out.good = 1;
  }
  SDSO_HD void finish_level() {
    out.lastResiduals[lvl] = sqrtf((float)(oldres[0] / oldres[1]));
    out.lastFlowIndicators[0] = oldres[2]; out.lastFlowIndicators[1] = oldres[3]; out.lastFlowIndicators[2] = oldres[4];
    if (trace.n < SDSO_TRACK_MAX_EVENTS) {        // the event, before the test: the second pass of a repeated level overwrites lastResiduals[lvl]
      const int e = trace.n++;
      trace.lvl[e] = lvl; trace.res[e] = out.lastResiduals[lvl];
      trace.flow[e][0] = oldres[2]; trace.flow[e][1] = oldres[3]; trace.flow[e][2] = oldres[4];
    }
    if (out.lastResiduals[lvl] > 1.5 * p.minResForAbort[lvl]) { done = true; return; }  // :1032 (good stays 0, pose untouched)
    if (levelCutoffRepeat > 1 && !haveRepeated) { lvl++; haveRepeated = true; }
    lvl--;
    if (lvl < 0) finish(); else start_level();
  }
  // Stage 1 of consuming an evaluation: the scalar decisions (:897-904, :1004-1023).  Returns 1 when an LM step has to be proposed
  // (then: if take_Hb copy H, b from the evaluation, solve_inc, propose_post); 0 when the next request (or `done`) is already set.
  SDSO_HD int consume_pre(const double* res, bool& take_Hb) {
    take_Hb = false;
    if (phase == 0) {
      for (int i = 0; i < 6; i++) oldres[i] = res[i];
      if (oldres[5] > 0.6 && levelCutoffRepeat < 50) { levelCutoffRepeat *= 2; request(cur, affCur); return 0; }   // :897-904
      take_Hb = true;
      lambda = 0.01f;
      iteration = 0;
    } else {
      const bool accept = (res[0] / res[1]) < (oldres[0] / oldres[1]);
      if (accept) {
        take_Hb = true;
        for (int i = 0; i < 6; i++) oldres[i] = res[i];
        affCur = affNew;
        cur = Tnew;
        lambda *= 0.5;
      } else {
        lambda *= 4;
        if (lambda < kLambdaExtrapolationLimit) lambda = kLambdaExtrapolationLimit;
      }
      double nrm = 0;
      for (int i = 0; i < 8; i++) nrm += inc[i] * inc[i];
      if (!(std::sqrt(nrm) > 1e-3)) { finish_level(); return 0; }
      iteration++;
    }
    if (iteration >= p.maxIterations[lvl]) { finish_level(); return 0; }
    out.iterations[lvl]++;
    return 1;
  }
  // Stage 2 (host form): inc from (H, b, lambda) and the affine modes (:931-964)
  SDSO_HD void solve_inc() {
    double* Hl = wHl; double* nb = wnb;
    for (int i = 0; i < 64; i++) Hl[i] = H[i];
    for (int i = 0; i < 8; i++) Hl[i * 8 + i] *= (1 + lambda);
    for (int i = 0; i < 8; i++) nb[i] = -b[i];
    solveLdltSmall(Hl, 8, 8, nb, inc, wwork, wperm);
    const bool fixA = p.affineOptModeA < 0, fixB = p.affineOptModeB < 0;
    if (!fixA && !fixB) return;
    // a fixed affine parameter: the reduced system's solution replaces the full one (:937-964)
    const double* Hm = Hl; const double* bm = nb;
    if (fixA && !fixB) {  // fix a alone: rows / columns 6 <- 7 (:949-964)
      double* Hs = wHs; double* bs = wbs;
      for (int i = 0; i < 64; i++) Hs[i] = Hl[i];
      for (int i = 0; i < 8; i++) bs[i] = -b[i];
      for (int i = 0; i < 8; i++) Hs[i * 8 + 6] = Hs[i * 8 + 7];
      for (int j = 0; j < 8; j++) Hs[6 * 8 + j] = Hs[7 * 8 + j];
      bs[6] = bs[7];
      Hm = Hs; bm = bs;
    }
    solveLdltSmall(Hm, 8, (fixA && fixB) ? 6 : 7, bm, wx, wwork, wperm);
    lm_place_reduced(fixA, fixB, wx, inc);
  }
  // Stage 3: extrapolation, scaling, SE3::exp and the request of the trial evaluation (:966-1000)
  SDSO_HD void propose_post() {
    double incScaled[8];
    lm_scale_step(lambda, inc, incScaled);
    Tnew = expSe3(incScaled) * cur;
    affNew = affCur;
    affNew.a += incScaled[6];
    affNew.b += incScaled[7];
    phase = 1;
    request(Tnew, affNew);
  }
  // host form of the whole consumption of one evaluation
  void consume(const TrackOut& O) {
    bool take = false;
    if (!consume_pre(O.res, take)) return;
    if (take) { for (int i = 0; i < 64; i++) H[i] = O.H[i]; for (int i = 0; i < 8; i++) b[i] = O.b[i]; }
    solve_inc();
    propose_post();
  }
};

// one hypothesis of the resident driver
struct LmJob {
  sdso_track_params_t p;
  const float4* pc[SDSO_PYR_LEVELS];
  const float4* img[SDSO_PYR_LEVELS];
  int n[SDSO_PYR_LEVELS];
  sdso_se3_t T;            // in: initial lastToNew; out: the call's result (unchanged when the call aborts, like the reference's references)
  sdso_aff_t aff;
  sdso_track_result_t out;
  sdso_track_trace_t trace;  // out: LmCore::trace (internal: no entry point but sdso_track_new_coarse reads it)
};
#ifndef LM_BLOCK_THREADS
#define LM_BLOCK_THREADS 512
#endif
#ifndef LM_UNROLL
#define LM_UNROLL 4
#endif
constexpr int LM_BLOCK = LM_BLOCK_THREADS;    // 512: 8 waves, the evaluation body wants ~200 VGPRs at four points per trip (two waves per SIMD)
}  // namespace sdso
