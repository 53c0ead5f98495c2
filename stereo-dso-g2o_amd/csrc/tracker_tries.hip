// FullSystem::trackNewCoarse STEP2-4 through the C-ABI: the ctx-free replay of the loop's rules and sdso_track_new_coarse (part of tracker.hip).
// The rules are track_tries.h; the tries run through track_newest_coarse_run (tracker_lm_api.hip), which hands back their event traces.
// The driver is stated once, over the runner of a batch: sdso_g2o_track_new_coarse (g2o_track_lm.hip) walks it with the fork-live runner.
#include "track_tries.h"
#include <vector>

extern "C" int sdso_track_tries_replay(int ntries, const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, sdso_track_try_t* recs,
                                       double* lastCoarseRMSE, double reTrackThreshold, sdso_track_tries_result_t* out) {
  if (!tries || !aff_last_2_l || !recs || !lastCoarseRMSE || !out) return SDSO_ERR_ARG;
  if (ntries < 1 || ntries > SDSO_TRACK_MAX_TRIES) return SDSO_ERR_ARG;
  for (int i = 0; i < ntries; i++) if (!track_trace_ok(recs[i].trace)) return SDSO_ERR_ARG;
  track_tries_replay(ntries, tries, *aff_last_2_l, recs, lastCoarseRMSE, reTrackThreshold, *out);
  return SDSO_OK;
}

int sdso::track_new_coarse_with(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries, const sdso_se3_t* tries,
                                const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold, sdso_track_tries_result_t* out,
                                sdso_track_try_t* recs, TrackBatchRunner runner) {
  if (!ctx) return SDSO_ERR_STATE;
  // ---- refusals: before any device work, nothing written
  SDSO_REQUIRE(ctx, prm && tries && aff_last_2_l && lastCoarseRMSE && out, "null argument");
  SDSO_REQUIRE(ctx, ntries >= 1 && ntries <= SDSO_TRACK_MAX_TRIES, "ntries out of range");
  SDSO_TRY(track_coarsest_level_ok(ctx, *prm));
  {
    LmJob probe;                                 // (the slots and every level the call walks, as the batch resolves them per hypothesis)
    SDSO_TRY(resolve_job(ctx, ref_slot, frame_slot, *prm, probe));
  }
  std::vector<sdso_track_try_t> own;
  if (!recs) { own.resize(ntries); recs = own.data(); }
  std::memset(recs, 0, sizeof(sdso_track_try_t) * (size_t)ntries);
  TrackTries S;
  S.init();
  // the tries i0 .. i0 + n - 1 in one launch under minResForAbort = S.achievedRes as it stands: the `in` members of their records
  auto run = [&](int i0, int n) -> int {
    std::vector<sdso_track_params_t> prms(n, *prm);
    std::vector<int> refs(n, ref_slot), frames(n, frame_slot);
    std::vector<sdso_se3_t> T(tries + i0, tries + i0 + n);
    std::vector<sdso_aff_t> aff(n, *aff_last_2_l);             // :442
    std::vector<sdso_track_result_t> outs(n);
    std::vector<sdso_track_trace_t> traces(n);
    for (int k = 0; k < n; k++) for (int l = 0; l < 5; l++) prms[k].minResForAbort[l] = S.achievedRes[l];
    SDSO_TRY(runner(ctx, n, refs.data(), frames.data(), prms.data(), T.data(), aff.data(), outs.data(), traces.data()));
    for (int k = 0; k < n; k++) {
      sdso_track_try_t& r = recs[i0 + k];
      r.trace.n = traces[k].n;                               // (member by member into the zeroed record: its bytes are a function of the events alone)
      for (int e = 0; e < traces[k].n && e < SDSO_TRACK_MAX_EVENTS; e++) {
        r.trace.lvl[e] = traces[k].lvl[e]; r.trace.res[e] = traces[k].res[e];
        for (int c = 0; c < 3; c++) r.trace.flow[e][c] = traces[k].flow[e][c];
      }
      r.end_good = outs[k].good; r.end_pose = T[k]; r.end_aff = aff[k];
    }
    return SDSO_OK;
  };
  // ---- phase 1: try 0 alone, the launch of the single call with NaN bounds; nearly every frame ends here (:499-500)
  SDSO_TRY(run(0, 1));
  bool stop = S.step(0, tries[0], *aff_last_2_l, lastCoarseRMSE[0], reTrackThreshold, recs[0]);
  // ---- phase 2: every other try in one launch under the bounds try 0 left (NaN where it was not good) — no tighter than the loop's own
  // at any later try, so each trace holds the events of the loop's try up to its abort; then the rules in list order
  if (!stop && ntries > 1) {
    SDSO_TRY(run(1, ntries - 1));
    int i = 1;
    for (; i < ntries && !stop; i++) stop = S.step(i, tries[i], *aff_last_2_l, lastCoarseRMSE[0], reTrackThreshold, recs[i]);
    for (; i < ntries; i++) std::memset(&recs[i], 0, sizeof(sdso_track_try_t));   // ran for nothing: the loop never saw them (ran = 0)
  }
  S.finish(tries[0], *aff_last_2_l, lastCoarseRMSE, *out);
  return SDSO_OK;
}

extern "C" int sdso_track_new_coarse(sdso_ctx* ctx, int ref_slot, int frame_slot, const sdso_track_params_t* prm, int ntries,
                                     const sdso_se3_t* tries, const sdso_aff_t* aff_last_2_l, double* lastCoarseRMSE, double reTrackThreshold,
                                     sdso_track_tries_result_t* out, sdso_track_try_t* recs) {
  return track_new_coarse_with(ctx, ref_slot, frame_slot, prm, ntries, tries, aff_last_2_l, lastCoarseRMSE, reTrackThreshold, out, recs,
                               track_newest_coarse_run);
}
