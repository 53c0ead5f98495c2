// The ctx-free host half of the BA window: everything about an uploaded (or edited) window that is decided from its integer arrays alone.
// Plain C++17 over the standard library and the ABI header — no HIP type, no ctx — so csrc/test_ba_layout.cpp checks it on a CPU.
//
//   build_window_layout  the range / order validations of an upload, the stable sort of the residuals by (host, target) pair, the
//                        per-point tables and the work lists of the accumulate and Schur kernels (ba_window.hip stages them as they are)
//   plan_window_edit     the integer list surgery of sdso_ba_window_update / sdso_ba_window_plan (ba_update.hip), O(np + nr)
//   plan_activated_stage7  stage 7 of such an edit from the records of an activation (sdso_ba_window_update_activated): integers only
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../include/sdso_abi.h"
#include "imm_layout.h"   // ImmActRec (plain C++ as well)

constexpr int BA_LAYOUT_CHUNK = 256;   // residuals per accumulate workgroup: BA_CHUNK of ba_kernels.h (checked where the chunks are staged)
constexpr int BA_LAYOUT_ITEM = 64;     // points per item of the Schur kernel (it deals 64-point slices to its waves)

// one entry of a work list, staged as an int4.  Chunk: {pair = host + target * nf, first sorted residual, count, 0};
// item: {host, first point, one past the last point, 0}
struct BaWorkItem { int x, y, z, w; };

struct WindowLayout {
  std::vector<int> perm, inv;                       // sorted -> window order, window order -> sorted
  std::vector<int> s_point;                         // the residual arrays in sorted order
  std::vector<uint8_t> s_host, s_target, s_state;
  std::vector<int> rbeg, rcnt;                      // per point: its first residual in window order (np + 1 entries), their number
  std::vector<unsigned> order;                      // per point: EFPoint::residualsAll order as target nibbles, 0xF behind the last (BaDev::p_order)
  std::vector<BaWorkItem> chunks, items;
  std::vector<int> pair_beg, host_beg;              // first chunk of every pair (nf * nf + 1), first item of every host (nf + 1)
  int host_pt_beg[9] = {0};                         // first point of every host; np from nf on
  int newest_first = 0;                             // first sorted residual whose target is the newest frame (nr: none)
  int have_first_frame = 0;                         // some frame of the window has frameID 0
};

static bool window_sizes_ok(const sdso_ba_window_t& Win, const char** why) {
  if (Win.nf >= 1 && Win.nf <= 8 && Win.np >= 0 && Win.nr >= 0) return true;
  *why = "window sizes out of range (nf <= 8: setting_maxFrames is 7, settings.cpp:65)";
  return false;
}

// Validate + sort the residuals by (host, target) pair, stable.  Two passes over the residuals (validation + keys + counts, then the
// placement with the sorted arrays written on the way) — a keyframe's upload is on the caller's critical path (round 5: ten passes and a
// np x nf scratch array were 66 of its 160 us).  Returns false with *why set; L is then unspecified.  Reads nf / np / nr, host,
// res_point / res_target / res_state and frameID of Win, nothing else.
static bool build_window_layout(const sdso_ba_window_t& Win, WindowLayout& L, const char** why) {
#define BAD(cond, msg) do { if (!(cond)) { *why = (msg); return false; } } while (0)
  if (!window_sizes_ok(Win, why)) return false;
  const int nf = Win.nf, np = Win.np, nr = Win.nr;
  L.have_first_frame = 0;
  for (int f = 0; f < nf; f++) if (Win.frameID[f] == 0) L.have_first_frame = 1;
  for (int p = 0; p < np; p++) {
    BAD(Win.host[p] >= 0 && Win.host[p] < nf, "point host out of range");
    BAD(p == 0 || Win.host[p] >= Win.host[p - 1], "points must be in allPoints order (host index non-decreasing)");
  }
  L.rbeg.assign(np + 1, 0); L.rcnt.assign(np, 0);
  std::vector<uint8_t> rkey(nr);
  int cnt[65] = {0};
  {
    int cur = -1; unsigned seen = 0;       // the targets the current point's residuals have named so far
    for (int i = 0; i < nr; i++) {
      const int p = Win.res_point[i], t = Win.res_target[i];
      BAD(p >= 0 && p < np && p >= cur, "residuals must be grouped by point in point order");
      BAD(t >= 0 && t < nf, "residual target out of range");
      if (p != cur) { cur = p; seen = 0; }
      BAD(!((seen >> t) & 1u), "two residuals of one point observe the same target frame");
      seen |= 1u << t;
      const int h = Win.host[p];
      // (the reference never creates one: `if(fh != point->host)`, FullSystemOptPoint.cpp:74; the Schur kernel has no column for it)
      BAD(t != h, "a residual observes its own host frame");
      BAD(++L.rcnt[p] <= SDSO_MAX_RES, "more than MAX_RES_PER_POINT residuals on a point");
      const int key = h + t * nf;           // htIDX (nf^2 <= 64 keys)
      rkey[i] = (uint8_t)key;
      cnt[key + 1]++;
    }
  }
  for (int p = 0; p < np; p++) L.rbeg[p + 1] = L.rbeg[p] + L.rcnt[p];     // (residuals are grouped by point: a point's first residual, nr behind the last)
  for (int k = 0; k < nf * nf; k++) cnt[k + 1] += cnt[k];
  int pair_first[65];
  for (int k = 0; k <= nf * nf; k++) pair_first[k] = cnt[k];          // first sorted residual of every pair (the chunk lists below)
  L.perm.resize(nr); L.inv.resize(nr);
  L.s_point.resize(nr); L.s_host.resize(nr); L.s_target.resize(nr); L.s_state.resize(nr);
  for (int i = 0; i < nr; i++) {            // stable counting sort: placement, the inverse and the sorted arrays in one pass
    const int key = rkey[i], j = cnt[key]++;
    L.perm[j] = i; L.inv[i] = j;
    L.s_point[j] = Win.res_point[i]; L.s_target[j] = (uint8_t)Win.res_target[i]; L.s_host[j] = (uint8_t)(key - L.s_target[j] * nf); L.s_state[j] = Win.res_state[i];
  }
  L.newest_first = nr > 0 ? std::min(pair_first[(nf - 1) * nf], nr) : nr;    // (keys host + target * nf)
  // EFPoint::residualsAll order of every point as a word of target nibbles; PointHessian::maxRelBaseline / numGoodResiduals
  L.order.assign(np, 0xffffffffu);
  for (int p = 0; p < np; p++)
    for (int k = 0; k < L.rcnt[p]; k++) L.order[p] = (L.order[p] & ~(15u << (4 * k))) | ((unsigned)Win.res_target[L.rbeg[p] + k] << (4 * k));
  // chunks per pair
  L.chunks.clear(); L.chunks.reserve(nf * nf + nr / BA_LAYOUT_CHUNK + 1);
  L.pair_beg.assign(nf * nf + 1, 0);
  for (int pair = 0; pair < nf * nf; pair++) {
    L.pair_beg[pair] = (int)L.chunks.size();
    const int start = pair_first[pair], j = pair_first[pair + 1];
    for (int s = start; s < j; s += BA_LAYOUT_CHUNK) L.chunks.push_back(BaWorkItem{pair, s, std::min(BA_LAYOUT_CHUNK, j - s), 0});
  }
  L.pair_beg[nf * nf] = (int)L.chunks.size();
  // point ranges per host, in 64-point items
  L.items.clear();
  L.host_beg.assign(nf + 1, 0);
  int p = 0;
  for (int h = 0; h <= 8; h++) {
    L.host_pt_beg[h] = p;
    if (h >= nf) continue;
    L.host_beg[h] = (int)L.items.size();
    while (p < np && Win.host[p] == h) p++;
    for (int s = L.host_pt_beg[h]; s < p; s += BA_LAYOUT_ITEM) L.items.push_back(BaWorkItem{h, s, std::min(s + BA_LAYOUT_ITEM, p), 0});
  }
  L.host_beg[nf] = (int)L.items.size();
  return true;
#undef BAD
}

struct WindowPlan {
  int nf2 = 0, np2 = 0, nr2 = 0;
  std::vector<int> frame_src, point_src, res_src;      // sdso_abi.h: index before the edit, or -1-k for the k-th appended entry
  std::vector<int> host, res_point, res_target;        // the edited window's integer arrays in its own numbering
  const char* why = nullptr;                           // the refusal
};

// The seven stages on plain index lists.  Returns false with P.why set for an edit the reference could not perform.
static bool plan_window_edit(int nf, int np, int nr, const int* host, const int* res_point, const int* res_target, const sdso_ba_window_edit_t& E, WindowPlan& P) {
#define BAD(cond, msg) do { if (!(cond)) { P.why = (msg); return false; } } while (0)
  BAD(nf >= 1 && nf <= 8 && np >= 0 && nr >= 0, "window sizes out of range");
  BAD((np == 0 || host) && (nr == 0 || (res_point && res_target)), "null window arrays");
  BAD(E.n_drop_res >= 0 && E.n_remove_points >= 0 && E.n_remove_frames >= 0 && E.n_add_frames >= 0 && E.n_add_res >= 0 && E.n_add_points >= 0 && E.n_pt_res >= 0, "negative count in the edit");
  BAD(E.n_add_frames <= 8 && E.n_drop_res <= nr && E.n_remove_points <= np && E.n_remove_frames <= nf, "a count of the edit exceeds what the window holds (at most 8 frames)");
  BAD(E.n_add_points <= (1 << 24) && E.n_add_res <= SDSO_MAX_RES * np && E.n_pt_res <= SDSO_MAX_RES * (long)E.n_add_points, "a count of the edit exceeds what the window can hold");
  BAD((!E.n_drop_res || E.drop_res) && (!E.n_remove_points || E.remove_points) && (!E.n_remove_frames || E.remove_frames), "null index list in the edit");
  BAD(!E.n_add_res || (E.add_res_point && E.add_res_target), "null stage-6 arrays");
  BAD(!E.n_add_points || E.pt_host, "null stage-7 hosts");
  BAD(!E.n_pt_res || (E.pt_res_point && E.pt_res_target), "null stage-7 residual arrays");
  const int nfa = nf + E.n_add_frames;                 // frames in the numbering before the call
  // ---- the window's lists (EFFrame::points with EFPoint::idxInPoints, EFPoint::residualsAll)
  std::vector<std::vector<int>> fpts(nfa);
  std::vector<int> pidx(np), rcnt(np, 0), rl((size_t)np * SDSO_MAX_RES);
  for (int f = 0; f < nfa; f++) fpts[f].reserve((size_t)np / nf + E.n_add_points + 16);
  for (int p = 0; p < np; p++) {
    BAD(host[p] >= 0 && host[p] < nf && (p == 0 || host[p] >= host[p - 1]), "point hosts out of range or not in allPoints order");
    pidx[p] = (int)fpts[host[p]].size();
    fpts[host[p]].push_back(p);
  }
  for (int r = 0; r < nr; r++) {
    const int p = res_point[r];
    BAD(p >= 0 && p < np && (r == 0 || p >= res_point[r - 1]) && res_target[r] >= 0 && res_target[r] < nf, "residuals out of range or not grouped by point");
    BAD(rcnt[p] < SDSO_MAX_RES, "more than MAX_RES_PER_POINT residuals on a point");
    rl[(size_t)p * SDSO_MAX_RES + rcnt[p]++] = r;
  }
  std::vector<uint8_t> ralive(nr, 1), palive(np, 1), falive(nfa, 1);
  auto target_of = [&](int id) { return id >= 0 ? res_target[id] : E.add_res_target[-1 - id]; };
  auto drop_at = [&](int p, int k) {                   // dropResidual (:529-533): the last entry takes the freed slot
    int* l = &rl[(size_t)p * SDSO_MAX_RES];
    l[k] = l[rcnt[p] - 1];
    rcnt[p]--;
  };
  auto remove_point = [&](int p) {                     // removePoint (:755-771)
    for (int k = 0; k < rcnt[p]; k++) ralive[rl[(size_t)p * SDSO_MAX_RES + k]] = 0;
    rcnt[p] = 0;
    std::vector<int>& L = fpts[host[p]];
    const int i = pidx[p], last = L.back();
    L[i] = last; pidx[last] = i;
    L.pop_back();
    palive[p] = 0;
  };
  // ---- stage 1
  for (int i = 0; i < E.n_drop_res; i++) {
    const int r = E.drop_res[i];
    BAD(r >= 0 && r < nr, "stage 1: residual index out of range");
    BAD(ralive[r], "stage 1: residual named twice");
    const int p = res_point[r];
    int k = 0;
    while (rl[(size_t)p * SDSO_MAX_RES + k] != r) k++;
    drop_at(p, k);
    ralive[r] = 0;
  }
  // ---- stage 2
  for (int i = 0; i < E.n_remove_points; i++) {
    const int p = E.remove_points[i];
    BAD(p >= 0 && p < np, "stage 2: point index out of range");
    BAD(palive[p], "stage 2: point named twice");
    remove_point(p);
  }
  // ---- stage 3
  if (E.drop_point) {
    for (int p = 0; p < np; p++) BAD(!E.drop_point[p] || palive[p], "stage 3: the point was already removed by stage 2");
    for (int f = 0; f < nf; f++)
      for (int i = 0; i < (int)fpts[f].size(); i++)    // dropPointsF (:741-747)
        if (E.drop_point[fpts[f][i]]) { remove_point(fpts[f][i]); i--; }
  }
  // ---- stage 4
  for (int i = 0; i < E.n_remove_frames; i++) {
    const int f = E.remove_frames[i];
    BAD(f >= 0 && f < nf, "stage 4: frame index out of range");
    BAD(falive[f], "stage 4: frame named twice");
    BAD(fpts[f].empty(), "stage 4: the frame still hosts a point (FullSystemMarginalize.cpp:148)");
    falive[f] = 0;
    for (int p = 0; p < np; p++) {
      if (!palive[p]) continue;
      for (int k = 0; k < rcnt[p]; k++) {
        const int r = rl[(size_t)p * SDSO_MAX_RES + k];
        if (res_target[r] == f) { drop_at(p, k); ralive[r] = 0; break; }
      }
    }
  }
  // ---- stage 5
  int nf2 = E.n_add_frames;
  for (int f = 0; f < nf; f++) nf2 += falive[f];
  BAD(nf2 <= 8, "more than 8 frames after the edit (setting_maxFrames is 7, settings.cpp:65)");
  BAD(nf2 >= 1, "no frame left after the edit");
  // ---- stage 6
  for (int i = 0; i < E.n_add_res; i++) {
    const int p = E.add_res_point[i], t = E.add_res_target[i];
    BAD(p >= 0 && p < np, "stage 6: point index out of range");
    BAD(palive[p], "stage 6: residual added to a point that leaves");
    BAD(t >= 0 && t < nfa, "stage 6: target frame out of range");
    BAD(falive[t], "stage 6: residual into a frame that leaves");
    BAD(t != host[p], "stage 6: a residual observes its own host frame");
    for (int k = 0; k < rcnt[p]; k++) BAD(target_of(rl[(size_t)p * SDSO_MAX_RES + k]) != t, "stage 6: the point already observes that target frame");
    BAD(rcnt[p] < SDSO_MAX_RES, "stage 6: more than MAX_RES_PER_POINT residuals on a point");
    rl[(size_t)p * SDSO_MAX_RES + rcnt[p]++] = -1 - i;
  }
  // ---- stage 7
  for (int i = 0; i < E.n_add_points; i++) {
    const int h = E.pt_host[i];
    BAD(h >= 0 && h < nfa, "stage 7: host frame out of range");
    BAD(falive[h], "stage 7: point hosted by a frame that leaves");
    fpts[h].push_back(-1 - i);
  }
  std::vector<int> prbeg(E.n_add_points + 1, 0);
  {
    unsigned seen = 0; int cur = -1;
    for (int i = 0; i < E.n_pt_res; i++) {
      const int q = E.pt_res_point[i], t = E.pt_res_target[i];
      BAD(q >= 0 && q < E.n_add_points && q >= cur, "stage 7: residual point index out of range or decreasing");
      if (q != cur) { cur = q; seen = 0; }
      BAD(t >= 0 && t < nfa, "stage 7: target frame out of range");
      BAD(falive[t], "stage 7: residual into a frame that leaves");
      BAD(t != E.pt_host[q], "stage 7: a residual observes its own host frame");
      BAD(!((seen >> t) & 1u), "stage 7: two residuals of one point observe the same target frame");
      seen |= 1u << t;
      BAD(++prbeg[q + 1] <= SDSO_MAX_RES, "stage 7: more than MAX_RES_PER_POINT residuals on a point");
    }
    for (int q = 0; q < E.n_add_points; q++) prbeg[q + 1] += prbeg[q];
  }
  // ---- makeIDX (:998-1018): frames, each frame's points, each point's residualsAll
  std::vector<int> fnew(nfa, -1);
  P.frame_src.clear();
  for (int f = 0; f < nfa; f++)
    if (falive[f]) { fnew[f] = (int)P.frame_src.size(); P.frame_src.push_back(f < nf ? f : -1 - (f - nf)); }
  const size_t np_max = (size_t)np + E.n_add_points, nr_max = (size_t)nr + E.n_add_res + E.n_pt_res;
  P.point_src.resize(np_max); P.host.resize(np_max); P.res_src.resize(nr_max); P.res_point.resize(nr_max); P.res_target.resize(nr_max);
  int p2 = 0, r2 = 0;
  for (int f = 0; f < nfa; f++) {
    if (!falive[f]) continue;
    for (int p : fpts[f]) {
      P.point_src[p2] = p;
      P.host[p2] = fnew[f];
      if (p >= 0) {
        const int* l = &rl[(size_t)p * SDSO_MAX_RES];
        for (int k = 0; k < rcnt[p]; k++, r2++) { P.res_src[r2] = l[k]; P.res_point[r2] = p2; P.res_target[r2] = fnew[target_of(l[k])]; }
      } else {
        for (int j = prbeg[-1 - p]; j < prbeg[-p]; j++, r2++) { P.res_src[r2] = -1 - (E.n_add_res + j); P.res_point[r2] = p2; P.res_target[r2] = fnew[E.pt_res_target[j]]; }
      }
      p2++;
    }
  }
  P.point_src.resize(p2); P.host.resize(p2); P.res_src.resize(r2); P.res_point.resize(r2); P.res_target.resize(r2);
  P.nf2 = nf2; P.np2 = (int)P.point_src.size(); P.nr2 = (int)P.res_src.size();
  return true;
#undef BAD
}

// Stage 7 of an edit from the records of sdso_imm_activate, by the tail of optimizeImmaturePoint (FullSystemOptPoint.cpp:196-237) and STEP 4
// of activatePointsMT (FullSystem.cpp:919-945): walking toOptimize in order, every record with status 1 is one appended point on host
// act_frame[rec.frame] (:923-928; the non-finite energyTH of :199-202 is already status -1), and for f = 0 .. nf_act-1 in frame order
// res_state[f] == IN is one residual into act_frame[f], state IN (:213-219; the host's own entry is 255).  Reads the integer members
// of the records only.  rec[k] = the toOptimize index of the k-th appended point.
struct ActStage7 {
  std::vector<int> pt_host, rec, res_point, res_target;
  std::vector<uint8_t> res_state;
};
// nf: frames of the window before the edit E (whose stages 4 and 5 are read); act_frame: nf_act indices in the edit's numbering.  Returns
// false with *why set for a map the call refuses: an entry outside [0, nf + n_add_frames), one that names a frame leaving in stage 4,
// two entries naming one frame.  What the plan itself refuses is left to plan_window_edit.
static bool plan_activated_stage7(int nf, const sdso_ba_window_edit_t& E, int nf_act, const int* act_frame, int n_rec, const sdso::ImmActRec* R, ActStage7& S,
                                  const char** why) {
#define BAD(cond, msg) do { if (!(cond)) { *why = (msg); return false; } } while (0)
  BAD(nf >= 1 && nf <= 8 && E.n_add_frames >= 0 && E.n_add_frames <= 8 && nf_act >= 0 && nf_act <= 8, "window or activation sizes out of range");
  const int nfa = nf + E.n_add_frames;
  unsigned leaving = 0, named = 0;
  if (E.remove_frames)
    for (int i = 0; i < E.n_remove_frames; i++) if (E.remove_frames[i] >= 0 && E.remove_frames[i] < nf) leaving |= 1u << E.remove_frames[i];
  for (int f = 0; f < nf_act; f++) {
    const int t = act_frame[f];
    BAD(t >= 0 && t < nfa, "act_frame: frame index out of range of the edited window");
    BAD(!((leaving >> t) & 1u), "act_frame: names a frame that leaves in stage 4");
    BAD(!((named >> t) & 1u), "act_frame: two activation frames mapped to one window frame");
    named |= 1u << t;
  }
  S = ActStage7();
  for (int p = 0; p < n_rec; p++) {
    const sdso::ImmActRec& r = R[p];
    if (r.status != 1) continue;
    BAD(r.frame >= 0 && r.frame < nf_act, "activation record names a frame outside the activation");
    const int q = (int)S.pt_host.size();
    S.pt_host.push_back(act_frame[r.frame]);
    S.rec.push_back(p);
    for (int f = 0; f < nf_act; f++)
      if (r.res_state[f] == 0) { S.res_point.push_back(q); S.res_target.push_back(act_frame[f]); S.res_state.push_back(0); }   // ResState::IN
  }
  return true;
#undef BAD
}
