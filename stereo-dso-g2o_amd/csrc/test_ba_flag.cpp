// CPU check of ba_flag.h: the per-point decision of removeOutliers / flagPointsForRemoval that k_ba_flag_points evaluates per lane.
// Stand-alone: includes only ba_flag.h, links nothing of the library.  tests/test_ba_flag_cpu.py builds and runs it:
//   g++ -std=c++17 -O1 test_ba_flag.cpp -o test_ba_flag && ./test_ba_flag
// and once under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_ba_flag.cpp -o test_ba_flag_san && ./test_ba_flag_san
// Every expectation below is read off the reference (FullSystem.cpp:965-1056, HessianBlocks.h:439-469, FullSystemOptimize.cpp:165-195,
// :1063-1084), not off the header.
#include "ba_flag.h"
#include <algorithm>
#include <cstdio>
#include <vector>

using namespace sdso;

static int g_failed = 0, g_checks = 0;
#define EXPECT(P, want_code, want_clause)                                                                                     \
  do {                                                                                                                        \
    int _cl = -1;                                                                                                             \
    const int _c = (P).decide(&_cl);                                                                                          \
    g_checks++;                                                                                                               \
    if (_c != (want_code) || _cl != (want_clause)) {                                                                          \
      std::printf("FAIL %s:%d: code %d (want %d), isOOB clause %d (want %d)\n", __FILE__, __LINE__, _c, (want_code), _cl, (want_clause)); \
      g_failed++;                                                                                                             \
    }                                                                                                                         \
  } while (0)

enum { IN = FLAG_RS_IN, OOB = FLAG_RS_OOB, OUTLIER = FLAG_RS_OUTLIER, NONE = FLAG_NONE };
struct Res { int target, state; bool removed; };

struct Point {
  int nf = 8, host = 0;
  unsigned marg = 0;                       // bit f: frame f is flaggedForMarginalization
  std::vector<Res> res;
  int gone[2] = {NONE, NONE};
  float idepth = 0.5f, idepth_hessian = 100.f;
  int numGood = 8;
  FlagSettings S{3, 4, 50.f};
  int decide(int* clause) const {
    FlagPointAcc a;
    for (const Res& r : res) flag_point_add(a, r.target, r.state, r.removed, nf, marg);
    return flag_point_decide(a.n, a.visInToMarg, flag_point_last(a.last[0], gone[0]), flag_point_last(a.last[1], gone[1]), idepth, numGood, idepth_hessian,
                             (marg >> host) & 1u, S, clause);
  }
};

// a healthy point hosted by frame 0 of 8: IN residuals into frames 7, 6 and 5, nothing flagged
static Point healthy() {
  Point P;
  P.res = {{7, IN, false}, {6, IN, false}, {5, IN, false}};
  return P;
}

int main() {
  {  // ---- KEEP, and the two early exits
    Point P = healthy();
    EXPECT(P, SDSO_PT_KEEP, 0);
    Point Q = P; Q.res.clear();
    EXPECT(Q, SDSO_PT_DROP_NO_RESIDUAL, 0);                         // removeOutliers: residuals.size() == 0
    Q = P; for (Res& r : Q.res) r.removed = true;
    EXPECT(Q, SDSO_PT_DROP_NO_RESIDUAL, 0);                         // every residual went to toRemove
    Q.idepth = -1.f;
    EXPECT(Q, SDSO_PT_DROP_NO_RESIDUAL, 0);                         // (removeOutliers runs first)
    Q = P; Q.idepth = -1e-6f;
    EXPECT(Q, SDSO_PT_DROP_NEGATIVE, 0);
    Q.idepth = -0.0f;
    EXPECT(Q, SDSO_PT_KEEP, 0);                                     // -0.0f < 0 is false
    Q.idepth = 0.0f;
    EXPECT(Q, SDSO_PT_KEEP, 0);
  }
  {  // ---- isOOB clause 1 alone (HessianBlocks.h:449-452): enough residuals, a long history, too few left outside the flagged frames
    Point P = healthy();
    P.marg = 1u << 5; P.numGood = 15;                               // 3 residuals, one IN into a flagged frame: 3 - 1 < 3
    EXPECT(P, SDSO_PT_MARGINALIZE, 1);
    Point Q = P; Q.numGood = 14;                                    // numGoodResiduals > 4 + 10 is strict
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res[2].state = OUTLIER;                                // only IN residuals count as visible in a flagged frame
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res.push_back({4, IN, false});                         // 4 - 1 >= 3
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q.marg |= 1u << 4;                                              // 4 - 2 < 3
    EXPECT(Q, SDSO_PT_MARGINALIZE, 1);
    Q = P; Q.res.pop_back(); Q.marg = 1u << 6;                      // n = 2 < minGoodActiveResForMarg: the clause needs n >= 3
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res[2].removed = true;                                 // a residual on toRemove is neither counted in n nor visible
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.idepth_hessian = 50.f;                                 // idepth_hessian > minIdepthH_marg is strict
    EXPECT(Q, SDSO_PT_DROP_WEAK, 1);
    Q.idepth_hessian = 50.000004f;
    EXPECT(Q, SDSO_PT_MARGINALIZE, 1);
  }
  {  // ---- isOOB clause 2 alone (:458): lastResiduals[0].second == OOB
    Point P = healthy();
    P.res[0].state = OOB;
    EXPECT(P, SDSO_PT_MARGINALIZE, 2);
    Point Q = P; Q.res[0].removed = true;                           // n = 2: not isInlierNew (n >= 3)
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 2);
    Q = P; Q.numGood = 4;                                           // isInlierNew: numGoodResiduals >= 4
    EXPECT(Q, SDSO_PT_MARGINALIZE, 2);
    Q.numGood = 3;
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 2);
    Q = P; Q.idepth_hessian = 49.f;
    EXPECT(Q, SDSO_PT_DROP_WEAK, 2);
    Q = healthy(); Q.res.erase(Q.res.begin());                      // no residual into the newest frame and no caller value: OOB (FullSystemOptPoint.cpp:204-207)
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 2);
    Q.gone[0] = NONE; Q.res.push_back({4, IN, false});
    EXPECT(Q, SDSO_PT_MARGINALIZE, 2);
    Q.gone[0] = IN;                                                 // the caller's history of a residual an earlier keyframe dropped
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = healthy(); Q.res = {{7, OOB, false}};                       // n = 1: clause 2 comes before `residuals.size() < 2`
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 2);
  }
  {  // ---- isOOB clause 3 alone (:459-460): both of the last two residuals are outliers, n >= 2
    Point P = healthy();
    P.res[0].state = OUTLIER; P.res[1].state = OUTLIER;
    EXPECT(P, SDSO_PT_MARGINALIZE, 3);
    Point Q = P; Q.res[1].state = IN;
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res[0].state = IN;
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res[2].removed = true;                                 // n = 2
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 3);
    Q.res[1].removed = true;                                        // n = 1: `residuals.size() < 2` returns false first
    EXPECT(Q, SDSO_PT_KEEP, 0);
    // a residual on toRemove still gives lastResiduals[k].second its state (FullSystemOptimize.cpp:167-173 run before :184-187)
    Q = healthy(); Q.res.push_back({4, IN, false}); Q.res[0] = {7, OUTLIER, true}; Q.res[1] = {6, OUTLIER, true};
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 3);                          // n = 2
    Q.res.push_back({3, IN, false});
    EXPECT(Q, SDSO_PT_MARGINALIZE, 3);
    Q.res[1].state = IN;                                            // OUTLIER (on toRemove) and IN (on toRemove): neither slot reads OOB, the point stays
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.res.erase(Q.res.begin() + 1);                          // no residual into frame nf-2: OOB, which is not OUTLIER
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q.gone[1] = OUTLIER;
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 3);                          // n = 2
  }
  {  // ---- the host frame is flagged, isOOB false (FullSystem.cpp:1004)
    Point P = healthy();
    P.host = 2; P.marg = 1u << 2;
    EXPECT(P, SDSO_PT_MARGINALIZE, 0);
    Point Q = P; Q.idepth_hessian = 50.f;
    EXPECT(Q, SDSO_PT_DROP_WEAK, 0);
    Q = P; Q.numGood = 3;
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 0);
    Q = P; Q.res[2].removed = true;
    EXPECT(Q, SDSO_PT_DROP_NOT_INLIER, 0);
    Q = P; Q.marg = 1u << 1;                                        // another frame flagged, none of the point's
    EXPECT(Q, SDSO_PT_KEEP, 0);
    Q = P; Q.idepth = -2.f;
    EXPECT(Q, SDSO_PT_DROP_NEGATIVE, 0);
  }
  {  // ---- a last_gone value beats a live residual, in both directions and in both slots
    Point P = healthy();
    P.gone[0] = OOB;
    EXPECT(P, SDSO_PT_MARGINALIZE, 2);
    P = healthy(); P.res[0].state = OOB; P.gone[0] = IN;
    EXPECT(P, SDSO_PT_KEEP, 0);
    P = healthy(); P.res[0].state = OUTLIER; P.gone[1] = OUTLIER;   // live IN into frame 6, caller says OUTLIER
    EXPECT(P, SDSO_PT_MARGINALIZE, 3);
    P.gone[1] = NONE;
    EXPECT(P, SDSO_PT_KEEP, 0);
  }
  {  // ---- nf = 2: frame 1 is the newest, frame 0 is frame nf-2
    Point P;
    P.nf = 2; P.host = 0; P.res = {{1, IN, false}};
    EXPECT(P, SDSO_PT_KEEP, 0);                                     // n = 1, last[0] = IN
    P.res[0].state = OOB;
    EXPECT(P, SDSO_PT_DROP_NOT_INLIER, 2);
    P.host = 1; P.res = {{0, IN, false}};                           // hosted by the newest frame: no residual into it, last[0] = OOB
    EXPECT(P, SDSO_PT_DROP_NOT_INLIER, 2);
    P.gone[0] = IN;
    EXPECT(P, SDSO_PT_KEEP, 0);
    P.marg = 1u << 0;                                               // its only residual is IN and into the flagged frame; n < 3: clause 1 is off
    EXPECT(P, SDSO_PT_KEEP, 0);
    P.marg = 1u << 1;
    EXPECT(P, SDSO_PT_DROP_NOT_INLIER, 0);
    P.S.minGoodActiveResForMarg = 1;                                // settings travel with the call
    EXPECT(P, SDSO_PT_MARGINALIZE, 0);
    P.marg = 1u << 0; P.numGood = 15;                               // 1 - 1 < 1
    EXPECT(P, SDSO_PT_MARGINALIZE, 1);
  }
  {  // ---- the walk does not depend on the order of the residuals (dropResidual's swap-with-last permutes residualsAll)
    Point P = healthy();
    P.res = {{7, OUTLIER, true}, {6, OUTLIER, false}, {5, IN, false}, {4, IN, false}, {3, OOB, true}, {2, IN, false}, {1, IN, false}};
    P.marg = (1u << 5) | (1u << 1); P.numGood = 20;
    int cl0 = -1;
    const int c0 = P.decide(&cl0);
    std::sort(P.res.begin(), P.res.end(), [](const Res& a, const Res& b) { return a.target < b.target; });
    int n_perm = 0;
    do {
      int cl = -1;
      if (P.decide(&cl) != c0 || cl != cl0) { std::printf("FAIL: the decision depends on the residual order\n"); g_failed++; break; }
      n_perm++;
    } while (std::next_permutation(P.res.begin(), P.res.end(), [](const Res& a, const Res& b) { return a.target < b.target; }));
    g_checks += n_perm;
    EXPECT(P, SDSO_PT_MARGINALIZE, 3);                              // n = 5, two visible in flagged frames: 5 - 2 >= 3, so clause 1 is off
  }
  if (g_failed) { std::printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
  std::printf("ba_flag ok (%d checks)\n", g_checks);
  return 0;
}
