// CPU check of imm_layout.h: the member table of a resident immature point, the remove order of activatePointsMT STEP 5 and its closed
// form.  Stand-alone: includes only imm_layout.h, links nothing of the library.  tests/test_imm_layout_cpu.py builds and runs it:
//   g++ -std=c++17 -O1 -Wall test_imm_layout.cpp -o test_imm_layout && ./test_imm_layout
// and once under the sanitizers (clean when this file was written):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_imm_layout.cpp -o test_imm_layout_san && ./test_imm_layout_san
#include "imm_layout.h"
#include <cstdio>
#include <vector>

using namespace sdso;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; return; } \
  } while (0)

// fixed-seed generator (xorshift32)
struct Rng {
  uint32_t s;
  explicit Rng(uint32_t seed) : s(seed) {}
  uint32_t next() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
};

// (a) the members are contiguous, in order, and fill kImmFloats; the member the gather derives for float c is the table's
static void check_members() {
  int o = 0;
  for (int m = 0; m < kImmMembers; m++) {
    CHECK(imm_member(m).off == o && imm_member(m).width >= 1);
    o += imm_member(m).width;
  }
  CHECK(o == kImmFloats);
  for (int c = 0; c < kImmFloats; c++) {
    int m = 0;
    while (c >= imm_member(m).off + imm_member(m).width) m++;
    const ImmMember M = imm_member_of_float(c);
    const int inner = c - M.off;
    CHECK(M.off == imm_member(m).off && M.width == imm_member(m).width && inner >= 0 && inner < M.width);
  }
}

// (b) the loop of FullSystem.cpp:948-957 on a vector of old indices; a flagged entry stands for the null pointer
static std::vector<int> reference_loop(const std::vector<uint8_t>& flags) {
  std::vector<int> v(flags.size());
  for (size_t i = 0; i < v.size(); i++) v[i] = (int)i;
  for (unsigned int i = 0; i < v.size(); i++)
    if (flags[v[i]]) { v[i] = v.back(); v.pop_back(); i--; }
  return v;
}
// (b) imm_remove_order is that loop; (c) the closed form, computed as sdso_imm_activate's kernels compute it — the prefix in 256 chunks
// with a serial pass over the chunk sums (k_imm_act_prefix), back[] by the survivors at indices >= m (k_imm_act_back), src[] by the final
// indices (k_imm_act_src) — gives the same order
static void check_order(const std::vector<uint8_t>& flags) {
  const int n = (int)flags.size();
  const std::vector<int> ref = reference_loop(flags);
  std::vector<int> src(n + 1, -7);
  const int m = imm_remove_order(n, flags.data(), src.data());
  CHECK(m == (int)ref.size() && src[n] == -7);
  for (int i = 0; i < m; i++) CHECK(src[i] == ref[i]);

  const int per = (n + 255) / 256;
  std::vector<int> chunk(256, 0), pref(n, 0);
  auto lo = [&](int t) { return t * per < n ? t * per : n; };
  auto hi = [&](int t) { return lo(t) + per < n ? lo(t) + per : n; };
  for (int t = 0; t < 256; t++)
    for (int k = lo(t); k < hi(t); k++) chunk[t] += flags[k];
  int nflag = 0;
  for (int t = 0; t < 256; t++) { const int c = chunk[t]; chunk[t] = nflag; nflag += c; }
  for (int t = 0; t < 256; t++) {
    int run = chunk[t];
    for (int k = lo(t); k < hi(t); k++) { pref[k] = run; run += flags[k]; }
  }
  int before = 0;
  for (int i = 0; i < n; i++) { CHECK(pref[i] == before); before += flags[i]; }
  CHECK(nflag == before && m == n - nflag);

  std::vector<int> back(n + 1, -1);
  int holes = 0, behind = 0;
  for (int i = 0; i < m; i++) holes += flags[i];
  for (int i = 0; i < n; i++) {
    if (flags[i] || i < m) continue;
    const int k = imm_back_slot(n, nflag, i, pref[i]);
    CHECK(k >= 0 && k < holes && back[k] == -1);   // every survivor behind m has a hole of its own in front of m
    back[k] = i;
    behind++;
  }
  CHECK(behind == holes);
  for (int i = 0; i < m; i++) CHECK(imm_final_src(i, flags[i] != 0, pref[i], back.data()) == ref[i]);
}

int main() {
  check_members();
  int patterns = 0;
  for (int n = 0; n <= 12; n++)
    for (unsigned bits = 0; bits < (1u << n); bits++, patterns++) {
      std::vector<uint8_t> f(n);
      for (int i = 0; i < n; i++) f[i] = (bits >> i) & 1;
      check_order(f);
    }
  if (patterns != 8191) { std::printf("FAIL: %d exhaustive patterns, expected 8191\n", patterns); g_failed++; }
  // the chunk edges of the 256-thread prefix and the window's own group size; flagged shares: none, all, 1/64, 1/8, 1/2, 7/8, 63/64
  Rng rng(0x1aa70e5du);
  const uint32_t share[7] = {0u, 0xffffffffu, 0x04000000u, 0x20000000u, 0x80000000u, 0xe0000000u, 0xfc000000u};
  for (int n : {255, 256, 257, 3000})
    for (int trial = 0; trial < 21; trial++) {
      std::vector<uint8_t> f(n);
      for (int i = 0; i < n; i++) f[i] = share[trial % 7] == 0xffffffffu || rng.next() < share[trial % 7];
      check_order(f);
    }
  if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
  std::printf("imm_layout ok\n");
  return 0;
}
