// CPU check of ba_layout.h: build_window_layout (what an upload validates, sorts and cuts into work lists) and its composition with
// plan_window_edit.  Stand-alone: includes only ba_layout.h, links nothing of the library.  tests/test_ba_layout_cpu.py builds and runs it:
//   g++ -std=c++17 -O1 test_ba_layout.cpp -o test_ba_layout && ./test_ba_layout
// and once under the sanitizers (clean when this file was written):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_ba_layout.cpp -o test_ba_layout_san && ./test_ba_layout_san
// Not covered: the "more than MAX_RES_PER_POINT residuals on a point" refusal — a point of a window of <= 8 frames that names no target
// twice and never its own host has at most 7 residuals, so an otherwise valid window cannot reach it (tests/test_window_plan_cpu.py says
// the same of the plan).
#include "ba_layout.h"
#include <cstdio>
#include <cstring>
#include <string>

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) { std::printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #cond); g_failed++; return; } \
  } while (0)

// fixed-seed generator (xorshift32)
struct Rng {
  uint32_t s;
  explicit Rng(uint32_t seed) : s(seed) {}
  uint32_t next() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

// the fields of sdso_ba_window_t that build_window_layout reads
struct Window {
  int nf = 0;
  std::vector<int> frameID, host, res_point, res_target;
  std::vector<uint8_t> res_state;
  sdso_ba_window_t view() const {
    sdso_ba_window_t W;
    std::memset(&W, 0, sizeof(W));
    W.nf = nf; W.np = (int)host.size(); W.nr = (int)res_point.size();
    W.frameID = frameID.data(); W.host = host.data();
    W.res_point = res_point.data(); W.res_target = res_target.data(); W.res_state = res_state.data();
    return W;
  }
  void add_point(int h, const std::vector<int>& targets, Rng& rng) {
    const int p = (int)host.size();
    host.push_back(h);
    for (int t : targets) { res_point.push_back(p); res_target.push_back(t); res_state.push_back((uint8_t)rng.below(3)); }
  }
};
static Window make_frames(int nf, int first_id) {
  Window W;
  W.nf = nf;
  for (int f = 0; f < nf; f++) W.frameID.push_back(first_id + f);
  return W;
}
// nf = 3, 700 points on host 0: every point observes target 1, every other one target 2 as well; hosts 1 and 2 are empty
static Window window_one_big_pair(Rng& rng) {
  Window W = make_frames(3, 0);
  for (int p = 0; p < 700; p++) W.add_point(0, (p & 1) ? std::vector<int>{1, 2} : std::vector<int>{1}, rng);
  return W;
}
// nf = 8, 40 points per host, a random non-empty subset of the other frames per point in random order
static Window window_random(Rng& rng) {
  Window W = make_frames(8, 5);
  for (int h = 0; h < 8; h++)
    for (int k = 0; k < 40; k++) {
      std::vector<int> ts;
      while (ts.empty())
        for (int t = 0; t < 8; t++) if (t != h && rng.below(2)) ts.push_back(t);
      for (int i = (int)ts.size() - 1; i > 0; i--) std::swap(ts[i], ts[rng.below(i + 1)]);
      W.add_point(h, ts, rng);
    }
  return W;
}

static void check_layout(const char* name, const Window& Wd) {
  g_case = name;
  const sdso_ba_window_t W = Wd.view();
  const int nf = W.nf, np = W.np, nr = W.nr;
  WindowLayout L;
  const char* why = nullptr;
  CHECK(build_window_layout(W, L, &why));
  // ---- permutation: perm / inv inverse of each other, keys non-decreasing, stable inside a key
  CHECK((int)L.perm.size() == nr && (int)L.inv.size() == nr);
  std::vector<int> seen(nr, 0);
  for (int j = 0; j < nr; j++) { CHECK(L.perm[j] >= 0 && L.perm[j] < nr); seen[L.perm[j]]++; CHECK(L.inv[L.perm[j]] == j); }
  for (int i = 0; i < nr; i++) CHECK(seen[i] == 1);
  auto key = [&](int i) { return Wd.host[Wd.res_point[i]] + Wd.res_target[i] * nf; };
  for (int j = 1; j < nr; j++) {
    CHECK(key(L.perm[j - 1]) <= key(L.perm[j]));
    if (key(L.perm[j - 1]) == key(L.perm[j])) CHECK(L.perm[j - 1] < L.perm[j]);
  }
  // ---- sorted arrays = inputs through perm
  CHECK((int)L.s_point.size() == nr && (int)L.s_host.size() == nr && (int)L.s_target.size() == nr && (int)L.s_state.size() == nr);
  for (int j = 0; j < nr; j++) {
    const int i = L.perm[j];
    CHECK(L.s_point[j] == Wd.res_point[i] && L.s_target[j] == Wd.res_target[i] && L.s_state[j] == Wd.res_state[i]);
    CHECK(L.s_host[j] == Wd.host[Wd.res_point[i]]);
  }
  // ---- chunks: per pair contiguous, <= BA_LAYOUT_CHUNK, all but the last full, covering exactly the key's range; none for an empty pair
  CHECK((int)L.pair_beg.size() == nf * nf + 1 && L.pair_beg[0] == 0 && L.pair_beg[nf * nf] == (int)L.chunks.size());
  int at = 0;   // first sorted residual of the pair
  for (int pair = 0; pair < nf * nf; pair++) {
    int cnt = 0;
    for (int i = 0; i < nr; i++) cnt += key(i) == pair;
    const int c0 = L.pair_beg[pair], c1 = L.pair_beg[pair + 1];
    CHECK(c1 - c0 == (cnt + BA_LAYOUT_CHUNK - 1) / BA_LAYOUT_CHUNK);
    int pos = at;
    for (int c = c0; c < c1; c++) {
      const BaWorkItem& ch = L.chunks[c];
      CHECK(ch.x == pair && ch.y == pos && ch.w == 0);
      CHECK(ch.z >= 1 && ch.z <= BA_LAYOUT_CHUNK && (c == c1 - 1 || ch.z == BA_LAYOUT_CHUNK));
      pos += ch.z;
    }
    CHECK(pos == at + cnt);
    for (int j = at; j < at + cnt; j++) CHECK(key(L.perm[j]) == pair);
    at += cnt;
  }
  CHECK(at == nr);
  // ---- items: per host they tile host_pt_beg[h] .. host_pt_beg[h + 1] in 64s
  CHECK((int)L.host_beg.size() == nf + 1 && L.host_beg[0] == 0 && L.host_beg[nf] == (int)L.items.size());
  CHECK(L.host_pt_beg[0] == 0);
  for (int h = 0; h <= 8; h++) {
    int first = 0;
    while (first < np && Wd.host[first] < h) first++;
    CHECK(L.host_pt_beg[h] == (h < nf ? first : np));
  }
  for (int h = 0; h < nf; h++) {
    int pos = L.host_pt_beg[h];
    for (int c = L.host_beg[h]; c < L.host_beg[h + 1]; c++) {
      const BaWorkItem& it = L.items[c];
      CHECK(it.x == h && it.y == pos && it.w == 0);
      CHECK(it.z == std::min(pos + BA_LAYOUT_ITEM, L.host_pt_beg[h + 1]) && it.z > it.y);
      pos = it.z;
    }
    CHECK(pos == L.host_pt_beg[h + 1]);
  }
  // ---- newest_first: the first sorted residual whose target is the newest frame
  int nfirst = nr;
  for (int j = nr - 1; j >= 0; j--) if (L.s_target[j] == nf - 1) nfirst = j;
  CHECK(L.newest_first == nfirst);
  int first_frame = 0;
  for (int f = 0; f < nf; f++) first_frame |= Wd.frameID[f] == 0;
  CHECK(L.have_first_frame == first_frame);
  // ---- point tables
  CHECK((int)L.rbeg.size() == np + 1 && (int)L.rcnt.size() == np && (int)L.order.size() == np);
  int r = 0;
  for (int p = 0; p < np; p++) {
    CHECK(L.rbeg[p] == r);
    int c = 0;
    while (r < nr && Wd.res_point[r] == p) { CHECK(((L.order[p] >> (4 * c)) & 15u) == (unsigned)Wd.res_target[r]); r++; c++; }
    CHECK(L.rcnt[p] == c);
    for (int k = c; k < 8; k++) CHECK(((L.order[p] >> (4 * k)) & 15u) == 15u);
  }
  CHECK(r == nr && L.rbeg[np] == nr);
}

static void check_big_pair_shape(const Window& Wd) {
  g_case = "one big pair: shape";
  const sdso_ba_window_t W = Wd.view();
  WindowLayout L;
  const char* why = nullptr;
  CHECK(build_window_layout(W, L, &why));
  const int pair = 0 + 1 * 3;   // host 0, target 1
  CHECK(L.pair_beg[pair + 1] - L.pair_beg[pair] == 3);
  CHECK(L.chunks[L.pair_beg[pair]].z == 256 && L.chunks[L.pair_beg[pair] + 1].z == 256 && L.chunks[L.pair_beg[pair] + 2].z == 188);
  CHECK(L.host_beg[1] - L.host_beg[0] == 11 && L.items[10].z - L.items[10].y == 60);
  CHECK(L.host_beg[1] == L.host_beg[2] && L.host_beg[2] == L.host_beg[3]);
}

static void check_refused(const char* name, const Window& Wd, const char* text, int nf_override = -1) {
  g_case = name;
  sdso_ba_window_t W = Wd.view();
  if (nf_override >= 0) W.nf = nf_override;
  WindowLayout L;
  const char* why = nullptr;
  CHECK(!build_window_layout(W, L, &why));
  CHECK(why && std::string(why) == text);
}

static void check_refusals(const Window& good) {
  const char* sizes = "window sizes out of range (nf <= 8: setting_maxFrames is 7, settings.cpp:65)";
  const char* grouped = "residuals must be grouped by point in point order";
  const int np = (int)good.host.size(), nr = (int)good.res_point.size();
  check_refused("nf = 0", good, sizes, 0);
  check_refused("nf = 9", good, sizes, 9);
  { Window W = good; W.host[np - 1] = W.nf; check_refused("host out of range", W, "point host out of range"); }
  { Window W = good; W.host[np - 1] = 0; check_refused("hosts decreasing", W, "points must be in allPoints order (host index non-decreasing)"); }
  { Window W = good; W.res_point[nr - 1] = np; check_refused("res_point out of range", W, grouped); }
  { Window W = good; W.res_point[nr - 1] = 0; check_refused("res_point decreasing", W, grouped); }
  { Window W = good; W.res_target[nr / 2] = W.nf; check_refused("target out of range", W, "residual target out of range"); }
  {
    Window W = good;
    int i = 1;
    while (W.res_point[i] != W.res_point[i - 1]) i++;
    W.res_target[i] = W.res_target[i - 1];
    check_refused("one target twice", W, "two residuals of one point observe the same target frame");
  }
  { Window W = good; W.res_target[nr / 2] = W.host[W.res_point[nr / 2]]; check_refused("own host", W, "a residual observes its own host frame"); }
}

// plan_window_edit on the random window: frame 0's points and frame 0 leave, one frame comes, 25 points hosted by it arrive with a residual
// into every other frame; what the plan hands to the upload must be a window the upload accepts
static void check_plan_composes(const Window& Wd, Rng& rng) {
  g_case = "plan_window_edit -> build_window_layout";
  const int nf = Wd.nf, np = (int)Wd.host.size(), nr = (int)Wd.res_point.size();
  std::vector<int> remove_points, remove_frames{0}, pt_host(25, nf), pt_res_point, pt_res_target;
  for (int p = 0; p < np; p++) if (Wd.host[p] == 0) remove_points.push_back(p);
  for (int q = 0; q < 25; q++)
    for (int t = 1; t < nf; t++) { pt_res_point.push_back(q); pt_res_target.push_back(t); }
  sdso_ba_window_edit_t E;
  std::memset(&E, 0, sizeof(E));
  E.n_remove_points = (int)remove_points.size(); E.remove_points = remove_points.data();
  E.n_remove_frames = 1; E.remove_frames = remove_frames.data();
  E.n_add_frames = 1;
  E.n_add_points = 25; E.pt_host = pt_host.data();
  E.n_pt_res = (int)pt_res_point.size(); E.pt_res_point = pt_res_point.data(); E.pt_res_target = pt_res_target.data();
  WindowPlan P;
  CHECK(plan_window_edit(nf, np, nr, Wd.host.data(), Wd.res_point.data(), Wd.res_target.data(), E, P));
  CHECK(P.nf2 == 8 && P.np2 == np - (int)remove_points.size() + 25);
  Window W2 = make_frames(P.nf2, 6);
  W2.host = P.host; W2.res_point = P.res_point; W2.res_target = P.res_target;
  for (int r = 0; r < P.nr2; r++) W2.res_state.push_back((uint8_t)rng.below(3));
  int into_new = 0;
  for (int r = 0; r < P.nr2; r++) into_new += W2.host[W2.res_point[r]] == 7;
  CHECK(into_new == 25 * 7);
  check_layout("plan_window_edit -> build_window_layout", W2);
}

int main() {
  Rng rng(0x5d50ba01u);
  { Window W = make_frames(1, 0); for (int p = 0; p < 3; p++) W.add_point(0, {}, rng); check_layout("nf = 1, np = 3, nr = 0", W); }
  check_layout("nf = 3, np = 0", make_frames(3, 2));
  const Window big = window_one_big_pair(rng);
  check_layout("one big pair", big);
  check_big_pair_shape(big);
  const Window rnd = window_random(rng);
  check_layout("nf = 8 random", rnd);
  check_refusals(rnd);
  check_plan_composes(rnd, rng);
  if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
  std::printf("ba_layout ok\n");
  return 0;
}
