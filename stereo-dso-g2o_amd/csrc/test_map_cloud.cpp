// CPU check of map_cloud.h: the keep tests, the vertex and the colour of KeyFrameDisplay::refreshPC that k_map_mark / k_map_emit evaluate per
// lane.  Stand-alone: includes only map_cloud.h, links nothing of the library.  tests/test_map_cloud_cpu.py builds and runs it:
//   g++ -std=c++17 -O1 -ffp-contract=off test_map_cloud.cpp -o test_map_cloud && ./test_map_cloud
// and once under the sanitizers:
//   g++ -std=c++17 -O1 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_map_cloud.cpp -o test_map_cloud_san
// Every expectation below is worked by hand from the reference (IOWrapper/Pangolin/KeyFrameDisplay.cpp:68-83, :104-160, :215-289), not read
// off the header; the bit patterns were computed one IEEE operation at a time.
#include "map_cloud.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace sdso;

static int g_failed = 0, g_checks = 0;
#define EXPECT_EQ(got, want)                                                                         \
  do {                                                                                               \
    const long long _g = (long long)(got), _w = (long long)(want);                                   \
    g_checks++;                                                                                      \
    if (_g != _w) { std::printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #got, _g, _w); g_failed++; } \
  } while (0)

static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
static float from_bits(uint32_t b) { float v; std::memcpy(&v, &b, 4); return v; }
#define EXPECT_BITS(got, want) EXPECT_EQ(bits(got), (uint32_t)(want))

// a point every clause passes in mode 1 with the thresholds below: depth = 2, depth^4 = 16, var = 1 / (0 + 0.01) = 100, var * depth^4 = 1600
struct Pt { int status = MAP_ST_ACTIVE; float idepth = 0.5f, idh = 0.f, bs = 0.25f; };
struct Th { int mode = 1; float scaled = 1600.f, abs = 100.f, minBS = 0.25f; };
static int clause(const Pt& p, const Th& t) { return map_drop_clause(p.status, p.idepth, p.idh, p.bs, t.mode, t.scaled, t.abs, t.minBS); }

int main() {
  const float NaN = std::numeric_limits<float>::quiet_NaN(), INF = std::numeric_limits<float>::infinity();
  {  // ---- :215-217, the mode / status table
    const int want[5][4] = {{0, 0, 0, 0},     // mode 0: all points
                            {1, 0, 0, 1},     // mode 1: active and marginalised
                            {1, 0, 1, 1},     // mode 2: active only
                            {1, 1, 1, 1},     // mode 3: nothing
                            {1, 1, 1, 1}};    // above 3: nothing
    for (int mode = 0; mode < 5; mode++)
      for (int st = 0; st < 4; st++) {
        Pt p; p.status = st;
        Th t; t.mode = mode;
        EXPECT_EQ(clause(p, t), want[mode][st]);
        EXPECT_EQ(map_keep(p.status, p.idepth, p.idh, p.bs, t.mode, t.scaled, t.abs, t.minBS), want[mode][st] == 0);
      }
    Pt p; p.status = MAP_ST_OUT;
    Th t; t.mode = -1;                        // none of the three tests names a negative mode
    EXPECT_EQ(clause(p, t), 0);
  }
  {  // ---- every threshold on both sides; each comparison is strict, so equality keeps
    Pt p; Th t;
    EXPECT_EQ(clause(p, t), 0);
    t = Th(); t.scaled = from_bits(0x44c7ffff);   // the float below 1600
    EXPECT_EQ(clause(p, t), 3);
    t = Th(); t.abs = from_bits(0x42c7ffff);      // the float below 100
    EXPECT_EQ(clause(p, t), 4);
    t = Th(); t.minBS = from_bits(0x3e800001);    // the float above 0.25
    EXPECT_EQ(clause(p, t), 5);
    p.bs = from_bits(0x3e7fffff);                  // the float below 0.25
    EXPECT_EQ(clause(p, Th()), 5);
    // the order of the clauses: a point that fails all of them reports the first
    p = Pt(); p.idepth = -0.5f; p.bs = 0.f; t = Th(); t.scaled = 1.f; t.abs = 1.f;
    EXPECT_EQ(clause(p, t), 2);
    p.idepth = 0.5f;
    EXPECT_EQ(clause(p, t), 3);
    t.scaled = 1600.f;
    EXPECT_EQ(clause(p, t), 4);
    t.abs = 100.f;
    EXPECT_EQ(clause(p, t), 5);
  }
  {  // ---- idepth 0, negative, -0, tiny
    Pt p; Th t;
    p.idepth = -1e-30f;
    EXPECT_EQ(clause(p, t), 2);
    p.idepth = 0.f;                                // depth = +inf, var * inf = inf > 1600
    EXPECT_EQ(clause(p, t), 3);
    t.scaled = INF;                                // inf > inf is false: the point is kept
    EXPECT_EQ(clause(p, t), 0);
    p.idepth = -0.f; t = Th();                     // -0 < 0 is false; depth = -inf, depth^4 = +inf
    EXPECT_EQ(clause(p, t), 3);
    p.idepth = 1e-30f;                             // depth = 1e30, depth * depth overflows
    EXPECT_EQ(clause(p, t), 3);
    t.scaled = INF;
    EXPECT_EQ(clause(p, t), 0);
  }
  {  // ---- idepth_hessian 0 gives var = 100 exactly (above); a large one, and inf, give a small var and 0
    Pt p; Th t;
    p.idh = 1e7f; t.scaled = 1e-5f; t.abs = 1e-6f;   // var ~ 1e-7, var * 16 ~ 1.6e-6
    EXPECT_EQ(clause(p, t), 0);
    t.abs = 1e-8f;
    EXPECT_EQ(clause(p, t), 4);
    p.idh = INF; t.scaled = 0.f; t.abs = 0.f;         // var = 0: 0 > 0 is false
    EXPECT_EQ(clause(p, t), 0);
    p.idh = -0.01f; t = Th();                         // (double)-0.01f + 0.01 is a tiny positive number: var is huge
    EXPECT_EQ(clause(p, t), 3);
  }
  {  // ---- a NaN passes every test it meets
    Pt p; Th t;
    p.idepth = NaN;
    EXPECT_EQ(clause(p, t), 0);
    p = Pt(); p.idh = NaN;
    EXPECT_EQ(clause(p, t), 0);
    p = Pt(); p.bs = NaN;
    EXPECT_EQ(clause(p, t), 0);
    // the immature record with idepth_max still NaN (:111-113): kept in mode 0 at minBS = 0, dropped by the baseline test above it
    const float id = map_immature_idepth(0.f, NaN);
    EXPECT_EQ(id != id, 1);
    EXPECT_EQ(map_drop_clause(MAP_ST_IMMATURE, id, MAP_IMMATURE_IDH, MAP_IMMATURE_BS, 0, 0.001f, 0.001f, 0.f), 0);
    EXPECT_EQ(map_drop_clause(MAP_ST_IMMATURE, id, MAP_IMMATURE_IDH, MAP_IMMATURE_BS, 0, 0.001f, 0.001f, 0.1f), 5);
    EXPECT_EQ(map_drop_clause(MAP_ST_IMMATURE, id, MAP_IMMATURE_IDH, MAP_IMMATURE_BS, 1, 0.001f, 0.001f, 0.f), 1);
    EXPECT_BITS(map_immature_idepth(1.f, 3.f), bits(2.f));
    EXPECT_BITS(MAP_IMMATURE_IDH, bits(1000.f));
    EXPECT_BITS(MAP_IMMATURE_BS, 0u);
  }
  {  // ---- :225: the quotient is formed in double and rounded once.  idepth_hessian = 4390.709 (0x458935ac): 1 / (h + 0.01) in double
     // rounds to 0x396ed104; float arithmetic (h + 0.01f, then 1.0f / that) gives 0x396ed105, one ulp above
    Pt p; p.idh = from_bits(0x458935ac);
    Th t; t.scaled = INF; t.abs = from_bits(0x396ed104);
    EXPECT_EQ(clause(p, t), 0);                       // var == absTH: kept.  The float quotient would be above it
    t.abs = from_bits(0x396ed103);
    EXPECT_EQ(clause(p, t), 4);
  }
  {  // ---- setFromF (:77-80) and the vertex (:244-246)
    const MapCalib K = map_calib(718.856f, 718.1f, 607.19f, 185.2f);
    EXPECT_BITS(K.fxi, 0x3ab6558b); EXPECT_BITS(K.fyi, 0x3ab686b0); EXPECT_BITS(K.cxi, 0xbf583bbc); EXPECT_BITS(K.cyi, 0xbe840bd6);
    float o[3];
    map_vertex(10.f, 20.f, 2.f, -2, 1, 0.5f, 0.25f, -1.f, -2.f, o);     // ((10 - 2) / 2 - 1) * 2, ((20 + 1) / 4 - 2) * 2
    EXPECT_BITS(o[0], bits(6.f)); EXPECT_BITS(o[1], bits(6.5f)); EXPECT_BITS(o[2], bits(2.f));
    const float depth = 1.0f / 0.3f;
    EXPECT_BITS(depth, 0x40555555);
    map_vertex(123.456f, 77.7f, depth, 1, -1, K.fxi, K.fyi, K.cxi, K.cyi, o);
    EXPECT_BITS(o[0], 0xc00f4289); EXPECT_BITS(o[1], 0xbf00eecd); EXPECT_BITS(o[2], 0x40555555);
    // the world transform: float, left to right.  Row 1 differs from the double sum rounded once (0xbf42ed91)
    const float T[12] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f, 1.5f, -2.25f, 10.125f};
    float w[3];
    map_to_world(T, o, w);
    EXPECT_BITS(w[0], 0xc00db651); EXPECT_BITS(w[1], 0xbf42ed90); EXPECT_BITS(w[2], 0x412ba6c9);
    // a NaN depth gives NaN in all three
    map_vertex(10.f, 20.f, NaN, 0, 0, 0.5f, 0.25f, -1.f, -2.f, o);
    EXPECT_EQ(o[0] != o[0] && o[1] != o[1] && o[2] != o[2], 1);
    // patternP = staticPattern[8] (settings.cpp:216)
    const int want[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};
    for (int k = 0; k < 8; k++) { int dx, dy; map_pattern(k, &dx, &dy); EXPECT_EQ(dx, want[k][0]); EXPECT_EQ(dy, want[k][1]); }
  }
  {  // ---- the colours (:250-289)
    const int want0[5][3] = {{0, 255, 255}, {0, 255, 0}, {0, 0, 255}, {255, 0, 0}, {255, 255, 255}};   // status 0..3, anything else
    for (int st = 0; st < 5; st++) {
      uint8_t c[3];
      map_colour(st == 4 ? 7 : st, 0, 99.f, c);
      for (int k = 0; k < 3; k++) EXPECT_EQ(c[k], want0[st][k]);
    }
    const struct { float c; int want; } grey[] = {{0.f, 0},      {0.99f, 0},  {1.f, 1},       {127.5f, 127}, {255.f, 255}, {255.9f, 255},
                                                  {256.f, 0},    {300.7f, 44}, {-0.5f, 0},    {-1.f, 255},   {-257.2f, 255}, {NaN, 0},
                                                  {1e10f, 0},    {-1e10f, 0},  {INF, 0},      {-INF, 0},     {2147483520.f, 128}};
    for (const auto& g : grey) {
      EXPECT_EQ(map_grey(g.c), g.want);
      for (int mode = 1; mode <= 2; mode++) {
        uint8_t c[3];
        map_colour(MAP_ST_ACTIVE, mode, g.c, c);
        EXPECT_EQ(c[0], g.want); EXPECT_EQ(c[1], g.want); EXPECT_EQ(c[2], g.want);
      }
    }
  }
  EXPECT_EQ(MAP_REC_FLOATS * sizeof(float), 64);
  EXPECT_EQ(MAP_COLOR + 8, MAP_PAD);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("map_cloud ok\n");
  return 0;
}
