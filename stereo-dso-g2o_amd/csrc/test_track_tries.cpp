// CPU check of track_tries.h: the loop over the motion tries of FullSystem::trackNewCoarse replayed from event traces.
// Stand-alone: includes only track_tries.h, links nothing of the library.  tests/test_track_tries_cpu.py builds and runs it:
//   g++ -std=c++17 -O1 test_track_tries.cpp -o test_track_tries && ./test_track_tries
// and once under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_track_tries.cpp -o test_track_tries_san && ./test_track_tries_san
// Every expectation below is read off the reference (FullSystem.cpp:436-511, CoarseTracker.cpp:855-856, :1029-1040), not off the header.
#include "track_tries.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace sdso;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    g_checks++;                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
  } while (0)

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

struct Ev { int lvl; double res; };
static sdso_se3_t pose_of(double tag) {
  sdso_se3_t T;
  for (int i = 0; i < 9; i++) T.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  T.t[0] = tag; T.t[1] = 0; T.t[2] = 0;
  return T;
}
// a try that starts at pose tag k and, un-aborted, ends at pose tag 100 + k with affine (k, -k); its flow indicators at event e are (k, e, 0)
static sdso_track_try_t make_try(int k, std::vector<Ev> ev, int end_good = 1) {
  sdso_track_try_t r;
  std::memset(&r, 0, sizeof(r));
  r.trace.n = (int)ev.size();
  for (int e = 0; e < r.trace.n; e++) { r.trace.lvl[e] = ev[e].lvl; r.trace.res[e] = ev[e].res; r.trace.flow[e][0] = k; r.trace.flow[e][1] = e; }
  r.end_good = end_good; r.end_pose = pose_of(100 + k); r.end_aff = {double(k), double(-k)};
  return r;
}

struct Loop {
  std::vector<sdso_track_try_t> recs;
  std::vector<sdso_se3_t> tries;
  sdso_aff_t aff0{0.25, -3.0};
  double rmse[5] = {0, 0, 0, 0, 0}, thr = 1.5;
  sdso_track_tries_result_t out;
  void add(std::vector<Ev> ev, int end_good = 1) { const int k = (int)recs.size(); recs.push_back(make_try(k, ev, end_good)); tries.push_back(pose_of(k)); }
  void run(double rmse0) {
    rmse[0] = rmse0;
    track_tries_replay((int)recs.size(), tries.data(), aff0, recs.data(), rmse, thr, out);
  }
};

int main() {
  const double N = NAN;
  {  // one good try from NaN bounds: it wins (!(res >= NaN)), achievedRes takes its residuals (:490 first operand), the level not used stays NaN
    Loop L; L.add({{3, 9}, {2, 8}, {1, 7}, {0, 6}});
    L.run(1e9);   // 6 < 1.5e9: the loop breaks after try 0
    CHECK(L.out.haveOneGood == 1 && L.out.winner == 0 && L.out.tryIterations == 1);
    CHECK(L.out.pose.t[0] == 100 && L.out.aff.a == 0 && L.out.flowVecs[0] == 0 && L.out.flowVecs[1] == 3);
    const double want[5] = {6, 7, 8, 9, N};
    for (int i = 0; i < 5; i++) { CHECK(same(L.out.achievedRes[i], want[i])); CHECK(same(L.rmse[i], want[i])); }
    CHECK(L.recs[0].ran == 1 && L.recs[0].good == 1 && L.recs[0].abort_lvl == -1 && L.recs[0].winner == 1);
  }
  {  // the stop rule on both sides of its threshold (:499, strict <): 6 < 4 * 1.5 is false, 6 < 4.0000001 * 1.5 is true; tries after the stop are not run
    for (int side = 0; side < 2; side++) {
      Loop L; L.add({{1, 7}, {0, 6}}); L.add({{1, 7}, {0, 5}});
      L.run(side ? 4.0000001 : 4.0);
      CHECK(L.out.tryIterations == (side ? 1 : 2) && L.out.winner == (side ? 0 : 1) && L.recs[1].ran == (side ? 0 : 1));
      CHECK(L.out.achievedRes[0] == (side ? 6 : 5));
    }
  }
  {  // a repeated level whose FIRST pass alone crosses the bound: level 2 ends at 13 > 1.5 * 8 = 12 and the call returns false there
     // (CoarseTracker.cpp:1032 comes before the repetition of :1036); the second pass (11, within the bound) never happens
    Loop L; L.add({{3, 9}, {2, 8}, {1, 7}, {0, 6}}); L.add({{3, 9}, {2, 13}, {2, 11}, {1, 7}, {0, 5}});
    L.run(0);
    const sdso_track_try_t& r = L.recs[1];
    CHECK(r.good == 0 && r.abort_lvl == 2 && r.winner == 0 && r.lastResiduals[2] == 13 && r.lastResiduals[3] == 9);
    CHECK(std::isnan(r.lastResiduals[1]) && std::isnan(r.lastResiduals[0]) && std::isnan(r.lastResiduals[4]));
    CHECK(r.pose.t[0] == 1 && r.aff.a == 0.25 && r.aff.b == -3.0);                     // the references stay untouched
    CHECK(r.lastFlowIndicators[0] == 1 && r.lastFlowIndicators[1] == 1);              // as written at the aborting event
    CHECK(L.out.winner == 0 && L.out.tryIterations == 2 && L.out.achievedRes[0] == 6 && L.out.achievedRes[2] == 8);
  }
  {  // ... and one whose SECOND pass alone crosses it: 11 passes, 13 aborts; lastResiduals[2] is the second pass'
    Loop L; L.add({{3, 9}, {2, 8}, {1, 7}, {0, 6}}); L.add({{3, 9}, {2, 11}, {2, 13}, {1, 7}, {0, 5}});
    L.run(0);
    CHECK(L.recs[1].good == 0 && L.recs[1].abort_lvl == 2 && L.recs[1].lastResiduals[2] == 13 && L.recs[1].lastFlowIndicators[1] == 2);
    CHECK(L.out.winner == 0);
  }
  {  // a repetition within the bound on both passes: the final residual is the second pass', and the try wins on level 0
    Loop L; L.add({{3, 9}, {2, 8}, {1, 7}, {0, 6}}); L.add({{3, 9}, {2, 11}, {2, 7.5}, {1, 7}, {0, 5}});
    L.run(0);
    CHECK(L.recs[1].good == 1 && L.recs[1].winner == 1 && L.recs[1].lastResiduals[2] == 7.5 && L.out.winner == 1);
    CHECK(L.out.achievedRes[2] == 7.5 && L.out.achievedRes[0] == 5 && L.out.pose.t[0] == 101);
  }
  {  // NaN bounds never abort (x > NaN is false): a first try that is not good leaves them NaN, the second runs through whatever its residuals
    Loop L; L.add({{1, 50}, {0, 40}}, 0); L.add({{1, 1e6}, {0, 1e5}});
    L.run(0);
    CHECK(L.recs[0].good == 0 && L.recs[0].abort_lvl == -1 && L.recs[0].pose.t[0] == 100);   // un-aborted: lastToNew_out is written even though the verdict is false (:1044)
    CHECK(L.recs[1].abort_lvl == -1 && L.recs[1].winner == 1 && L.out.winner == 1 && L.out.achievedRes[0] == 1e5 && L.out.achievedRes[1] == 1e6);
  }
  {  // a non-finite level-0 residual never wins (:476), also as a float overflow: (float)1e39 is inf
    Loop L; L.add({{1, 7}, {0, INFINITY}}); L.add({{1, 7}, {0, 1e39}}); L.add({{1, 7}, {0, N}});
    L.run(0);
    CHECK(L.out.haveOneGood == 0 && L.out.winner == -1 && L.out.tryIterations == 3);
    for (int i = 0; i < 5; i++) CHECK(std::isnan(L.out.achievedRes[i]));             // no carry before a good one (:487)
    CHECK(L.out.pose.t[0] == 0 && L.out.aff.a == 0.25 && L.out.aff.b == -3.0 && L.out.flowVecs[0] == 0 && L.out.flowVecs[1] == 0 && L.out.flowVecs[2] == 0);   // :503-508
  }
  {  // a residual equal to the bound: >= holds, no new winner (:477); the carry's strict > leaves the bound as it is
    Loop L; L.add({{1, 7}, {0, 6}}); L.add({{1, 6.5}, {0, 6}});
    L.run(0);
    CHECK(L.out.winner == 0 && L.recs[1].good == 1 && L.recs[1].winner == 0 && L.out.achievedRes[0] == 6 && L.out.achievedRes[1] == 6.5);
    CHECK(L.out.pose.t[0] == 100);
  }
  {  // an aborted try lowers a coarser bound: level 3 at 4 (< 9) is carried, the abort on level 2 (13 > 12) leaves levels 2..0 NaN, and a
     // NaN residual never lowers a bound (bound > NaN is false)
    Loop L; L.add({{3, 9}, {2, 8}, {1, 7}, {0, 6}}); L.add({{3, 4}, {2, 13}, {1, 1}, {0, 1}}); L.add({{3, 6.5}, {2, 8}});
    L.run(0);
    CHECK(L.recs[1].abort_lvl == 2 && L.recs[1].good == 0);
    CHECK(L.recs[2].abort_lvl == 3 && L.recs[2].lastResiduals[3] == 6.5);             // 6.5 > 1.5 * 4: the bound the aborted try lowered
    const double want[5] = {6, 7, 8, 4, N};
    for (int i = 0; i < 5; i++) CHECK(same(L.out.achievedRes[i], want[i]));
    CHECK(L.out.winner == 0 && L.out.tryIterations == 3);
  }
  {  // no good try at all: pose = tries[0], aff = aff_last_2_l, flow 0, achievedRes all NaN (:503-511)
    Loop L; L.add({{1, 7}, {0, 6}}, 0); L.add({{1, 7}, {0, 5}}, 0);
    L.run(1e9);
    CHECK(L.out.haveOneGood == 0 && L.out.winner == -1 && L.out.tryIterations == 2 && L.out.pose.t[0] == 0 && L.out.aff.a == 0.25);
    for (int i = 0; i < 5; i++) CHECK(std::isnan(L.rmse[i]));
  }
  {  // a try without events (cannot happen on the device; the replay is total): all NaN, flow 1000 (CoarseTracker.cpp:855-856)
    Loop L; L.add({});
    L.run(0);
    CHECK(L.recs[0].lastFlowIndicators[2] == 1000 && std::isnan(L.recs[0].lastResiduals[0]) && L.out.haveOneGood == 0);
  }
  {  // the trace check of the entry point
    sdso_track_trace_t t;
    std::memset(&t, 0, sizeof(t));
    CHECK(track_trace_ok(t));
    t.n = 7; CHECK(!track_trace_ok(t));
    t.n = -1; CHECK(!track_trace_ok(t));
    t.n = 6; t.lvl[5] = 5; CHECK(!track_trace_ok(t));
    t.lvl[5] = 4; CHECK(track_trace_ok(t));
    t.lvl[0] = -1; CHECK(!track_trace_ok(t));
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("track_tries ok\n");
  return 0;
}
