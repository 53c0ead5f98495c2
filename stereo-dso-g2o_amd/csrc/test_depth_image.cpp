// CPU check of depth_image.h: the statements of debugPlotIDepthMap that the kernels of depth_image.hip evaluate per lane.
// Stand-alone: includes only depth_image.h, links nothing of the library.  tests/test_depth_image_ref.py builds and runs it:
//   g++ -std=c++17 -O1 test_depth_image.cpp -o test_depth_image && ./test_depth_image
// and once under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_depth_image.cpp -o test_depth_image_san && ./test_depth_image_san
// The expectations are read off the reference (CoarseTracker.cpp:1078-1163, globalFuncs.h:362-379, MinimalImage.h:100-112): the overlay is
// compared with the literal scatter loop, makeJet3B with colours worked out by hand from its lines, the selection with std::sort.
#include "depth_image.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace sdso;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    g_checks++;                                                                \
    if (!(cond)) {                                                             \
      std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);             \
      std::printf(__VA_ARGS__);                                                \
      std::printf("\n");                                                       \
      g_failed++;                                                              \
    }                                                                          \
  } while (0)

// ------------------------------------------------------------------ the ring and the candidate order
static void test_ring() {
  // setPixelCirc's statements (MinimalImage.h:101-111) on a 7x7 block around (3, 3)
  bool lit[7][7] = {};
  const int u = 3, v = 3;
  for (int i = -3; i <= 3; i++) {
    lit[v + i][u + 3] = true; lit[v + i][u - 3] = true; lit[v + i][u + 2] = true; lit[v + i][u - 2] = true;
    lit[v - 3][u + i] = true; lit[v + 3][u + i] = true; lit[v - 2][u + i] = true; lit[v + 2][u + i] = true;
  }
  int n = 0;
  for (int dy = -4; dy <= 4; dy++)
    for (int dx = -4; dx <= 4; dx++) {
      const bool want = dx >= -3 && dx <= 3 && dy >= -3 && dy <= 3 && lit[3 + dy][3 + dx];
      CHECK(depth_ring(dx, dy) == want, "dx %d dy %d", dx, dy);
      n += want;
    }
  CHECK(n == DEPTH_RING_N, "%d ring pixels", n);
  // the candidates: each ring cell once, sources in strictly descending raster order (source = output - offset)
  bool seen[7][7] = {};
  int py = 0, px = 0;
  for (int k = 0; k < DEPTH_RING_N; k++) {
    int dx = 99, dy = 99;
    depth_ring_offset(k, &dx, &dy);
    CHECK(depth_ring(dx, dy), "candidate %d = (%d, %d) is not on the ring", k, dx, dy);
    if (!depth_ring(dx, dy)) continue;
    CHECK(!seen[dy + 3][dx + 3], "candidate %d repeats (%d, %d)", k, dx, dy);
    seen[dy + 3][dx + 3] = true;
    const int sy = -dy, sx = -dx;
    if (k) CHECK(sy < py || (sy == py && sx < px), "candidate %d (source %d, %d) does not precede candidate %d (source %d, %d) in raster order", k, sx, sy, k - 1, px, py);
    py = sy; px = sx;
  }
}

// ------------------------------------------------------------------ the gather against the literal scatter of :1129-1163
static void scatter_literal(const std::vector<float>& map, int w, int h, float minID, float maxID, std::vector<Rgb8>& img, int* circles) {
  *circles = 0;
  const int wl = w;
  for (int y = 3; y < h - 3; y++)
    for (int x = 3; x < wl - 3; x++) {
      const float* bp = map.data() + x + y * wl;
      float sid = 0, nid = 0;
      if (bp[0] > 0) { sid += bp[0]; nid++; }
      if (bp[1] > 0) { sid += bp[1]; nid++; }
      if (bp[-1] > 0) { sid += bp[-1]; nid++; }
      if (bp[wl] > 0) { sid += bp[wl]; nid++; }
      if (bp[-wl] > 0) { sid += bp[-wl]; nid++; }
      if (bp[0] > 0 || nid >= 3) {
        const float id = ((sid / nid) - minID) / ((maxID - minID));
        const Rgb8 val = make_jet_3b(id);
        (*circles)++;
        auto at = [&](int uu, int vv) -> Rgb8& { return img[(size_t)uu + (size_t)vv * w]; };
        for (int i = -3; i <= 3; i++) {   // setPixelCirc
          at(x + 3, y + i) = val; at(x - 3, y + i) = val; at(x + 2, y + i) = val; at(x - 2, y + i) = val;
          at(x + i, y - 3) = val; at(x + i, y + 3) = val; at(x + i, y - 2) = val; at(x + i, y + 2) = val;
        }
      }
    }
}
static void gather(const std::vector<float>& map, int w, int h, float minID, float maxID, std::vector<Rgb8>& img, int* circles) {
  *circles = 0;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      Rgb8 c;
      if (depth_source_inside(x, y, w, h)) {
        const float* bp = map.data() + x + y * w;
        if (depth_source(bp[0], bp[1], bp[-1], bp[w], bp[-w], minID, maxID, &c)) (*circles)++;
      }
      for (int k = 0; k < DEPTH_RING_N; k++) {
        int dx, dy;
        depth_ring_offset(k, &dx, &dy);
        const int sx = x - dx, sy = y - dy;
        if (!depth_source_inside(sx, sy, w, h)) continue;
        const float* bp = map.data() + sx + sy * w;
        if (depth_source(bp[0], bp[1], bp[-1], bp[w], bp[-w], minID, maxID, &c)) { img[(size_t)x + (size_t)y * w] = c; break; }
      }
    }
}
static void test_gather() {
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  const int shapes[][2] = {{6, 6}, {7, 7}, {8, 9}, {13, 11}, {31, 17}, {40, 33}, {70, 25}};
  const float fill[] = {0.02f, 0.1f, 0.3f, 0.7f, 1.0f};
  for (const auto& s : shapes)
    for (float p : fill)
      for (int rep = 0; rep < 3; rep++) {
        const int w = s[0], h = s[1];
        std::vector<float> map((size_t)w * h);
        for (float& v : map) v = U(rng) < p ? 0.05f + 1.95f * U(rng) : -1.f;
        if (rep == 1) map[map.size() / 2] = std::numeric_limits<float>::quiet_NaN();
        float lo = 0.3f, hi = 1.5f;
        if (rep == 2) lo = hi = 0.8f;   // id = +-inf / NaN
        std::vector<Rgb8> a((size_t)w * h, Rgb8{{7, 7, 7}}), b = a;
        int ca = -1, cb = -1;
        scatter_literal(map, w, h, lo, hi, a, &ca);
        gather(map, w, h, lo, hi, b, &cb);
        CHECK(ca == cb, "%dx%d fill %g: %d circles, gather counts %d", w, h, p, ca, cb);
        CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(Rgb8)) == 0, "%dx%d fill %g rep %d: gather differs from the scatter", w, h, p, rep);
      }
}

// ------------------------------------------------------------------ makeJet3B
static void expect_jet(float id, int r, int g, int b, int line) {
  const Rgb8 c = make_jet_3b(id);
  g_checks++;
  if (c.c[0] != r || c.c[1] != g || c.c[2] != b) {
    std::printf("FAIL line %d: makeJet3B(%.9g) = (%d, %d, %d), want (%d, %d, %d)\n", line, id, c.c[0], c.c[1], c.c[2], r, g, b);
    g_failed++;
  }
}
#define JET(id, r, g, b) expect_jet(id, r, g, b, __LINE__)
static float below(float v) { return std::nextafter(v, 0.f); }
static void test_jet() {
  const float inf = std::numeric_limits<float>::infinity();
  JET(std::numeric_limits<float>::quiet_NaN(), 255, 255, 255);   // (int)(NaN*8) = INT_MIN on x86: no case, :378
  JET(-inf, 128, 0, 0); JET(-1.f, 128, 0, 0); JET(-0.f, 128, 0, 0); JET(0.f, 128, 0, 0);   // :363
  JET(inf, 0, 0, 128); JET(1.f, 0, 0, 128); JET(7.f, 0, 0, 128);                            // :364
  // ifP = 0 at k/8; ifP = 1 - eps just below: 255*0.5 = 127.5 -> 127, 255*(0.5 + 0.5*(1-eps)) -> 254
  JET(std::numeric_limits<float>::denorm_min(), 127, 0, 0);   // icP 0: 255*(0.5+0.5*ifP)
  JET(0.0625f, 191, 0, 0);                                    //        ifP 0.5: 191.25
  JET(below(0.125f), 254, 0, 0);
  JET(0.125f, 255, 0, 0);                                     // icP 1: (255, 255*(0.5*ifP), 0)
  JET(below(0.25f), 255, 127, 0);
  JET(0.25f, 255, 127, 0);                                    // icP 2: (255, 255*(0.5+0.5*ifP), 0)
  JET(below(0.375f), 255, 254, 0);
  JET(0.375f, 255, 255, 0);                                   // icP 3: (255*(1-0.5*ifP), 255, 255*(0.5*ifP))
  JET(0.4375f, 191, 255, 63);                                 //        ifP 0.5: 191.25, 63.75
  JET(below(0.5f), 127, 255, 127);
  JET(0.5f, 127, 255, 127);                                   // icP 4: (255*(0.5-0.5*ifP), 255, 255*(0.5+0.5*ifP))
  JET(below(0.625f), 0, 255, 254);
  JET(0.625f, 0, 255, 255);                                   // icP 5: (0, 255*(1-0.5*ifP), 255)
  JET(below(0.75f), 0, 127, 255);
  JET(0.75f, 0, 127, 255);                                    // icP 6: (0, 255*(0.5-0.5*ifP), 255)
  JET(below(0.875f), 0, 0, 255);
  JET(0.875f, 0, 0, 255);                                     // icP 7: (0, 0, 255*(1-0.5*ifP))
  JET(below(1.f), 0, 0, 127);
}

// ------------------------------------------------------------------ the selection against std::sort (:1084-1088)
static float radix_select(const std::vector<float>& all, int which, int* count_out) {
  uint32_t prefix = 0;
  unsigned rank = 0;
  int count = 0;
  for (int pass = 0; pass < DEPTH_SEL_PASSES; pass++) {
    std::vector<unsigned> hist(DEPTH_SEL_BINS, 0);
    for (float v : all) {
      if (!depth_in_range_set(v)) continue;
      const uint32_t key = depth_key(v);
      if (pass == 0 || depth_sel_prefix(key, pass) == prefix) hist[depth_sel_digit(key, pass)]++;
    }
    if (pass == 0) {
      for (unsigned c : hist) count += (int)c;
      if (count == 0) { *count_out = 0; return -1.f; }
      rank = (unsigned)depth_range_rank(count, which);
    }
    unsigned excl = 0;
    for (int b = 0; b < DEPTH_SEL_BINS; b++) {
      if (rank < excl + hist[b]) { prefix = (prefix << depth_sel_bits(pass)) | (unsigned)b; rank -= excl; break; }
      excl += hist[b];
    }
  }
  *count_out = count;
  return depth_from_key(prefix);
}
static void test_select() {
  int bits = 0;
  for (int p = 0; p < DEPTH_SEL_PASSES; p++) {
    bits += depth_sel_bits(p);
    CHECK((1 << depth_sel_bits(p)) <= DEPTH_SEL_BINS, "pass %d", p);
    CHECK(depth_sel_shift(p) == 31 - bits, "pass %d: shift %d", p, depth_sel_shift(p));
  }
  CHECK(bits == 31, "%d bits", bits);
  std::mt19937 rng(99);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  const int sizes[] = {1, 2, 3, 19, 20, 21, 22, 100, 1000, 20001};
  for (int n : sizes)
    for (int kind = 0; kind < 4; kind++) {
      std::vector<float> all;
      for (int i = 0; i < n; i++) {
        float v = 0.05f + 1.95f * U(rng);
        if (kind == 1) v = std::ldexp(U(rng) + 1e-3f, (int)(U(rng) * 250) - 140);   // every exponent, denormals included
        if (kind == 2) v = 0.25f * (float)(1 + (int)(U(rng) * 5));                   // many ties
        if (kind == 3 && i % 7 == 0) v = i % 14 ? std::numeric_limits<float>::infinity() : 1e-42f;
        all.push_back(v);
        if (i % 3 == 0) all.push_back(-1.f);                                       // not members of allID
        if (i % 11 == 0) all.push_back(std::numeric_limits<float>::quiet_NaN());
        if (i % 13 == 0) all.push_back(0.f);
      }
      std::vector<float> allID;
      for (float v : all) if (v > 0) allID.push_back(v);
      std::sort(allID.begin(), allID.end());
      // keys order as the floats
      for (size_t i = 1; i < allID.size() && i < 2000; i++) CHECK(depth_key(allID[i - 1]) <= depth_key(allID[i]), "key order at %zu", i);
      const int nn = (int)allID.size() - 1;
      const float want[2] = {allID[(int)(nn * 0.05)], allID[(int)(nn * 0.95)]};
      for (int which = 0; which < 2; which++) {
        int count = -1;
        const float got = radix_select(all, which, &count);
        CHECK(count == (int)allID.size(), "n %d kind %d: count %d", n, kind, count);
        CHECK(depth_key(got) == depth_key(want[which]), "n %d kind %d which %d: %.9g, std::sort gives %.9g", n, kind, which, got, want[which]);
      }
    }
  int count = -1;
  radix_select({-1.f, 0.f, std::numeric_limits<float>::quiet_NaN()}, 0, &count);
  CHECK(count == 0, "empty: %d", count);
}

// ------------------------------------------------------------------ smoothing (:1090-1117) and background (:1123-1125)
static void test_smooth_background() {
  auto ref = [](float minID, float maxID, float* minID_pt, float* maxID_pt, float out[2]) {   // the reference's lines
    if (minID_pt != 0 && maxID_pt != 0) {
      if (*minID_pt < 0 || *maxID_pt < 0) { *maxID_pt = maxID; *minID_pt = minID; }
      else {
        float maxChange = 0.3 * (*maxID_pt - *minID_pt);
        if (minID < *minID_pt - maxChange) minID = *minID_pt - maxChange;
        if (minID > *minID_pt + maxChange) minID = *minID_pt + maxChange;
        if (maxID < *maxID_pt - maxChange) maxID = *maxID_pt - maxChange;
        if (maxID > *maxID_pt + maxChange) maxID = *maxID_pt + maxChange;
        *maxID_pt = maxID; *minID_pt = minID;
      }
    }
    out[0] = minID; out[1] = maxID;
  };
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float cases[][4] = {{0.1f, 1.9f, -1.f, -1.f}, {0.1f, 1.9f, 0.2f, -1.f}, {0.1f, 5.f, 1.f, 2.f}, {1.5f, 1.6f, 0.1f, 1.f}, {0.11f, 1.01f, 0.1f, 1.f},
                             {0.7f, 0.7f, 0.7f, 0.7f}, {0.3f, 0.9f, nan, 1.f}, {0.3f, 0.9f, 2.f, 1.f}, {0.05f, 0.06f, 0.123456f, 7.654321f}};
  for (const auto& c : cases) {
    float a = c[2], b = c[3], want[2], got[2];
    ref(c[0], c[1], &a, &b, want);
    const float prev[2] = {c[2], c[3]};
    depth_range_smooth(c[0], c[1], true, prev, got);
    CHECK(depth_key(got[0]) == depth_key(want[0]) && depth_key(got[1]) == depth_key(want[1]), "smooth (%g, %g) against (%g, %g): (%.9g, %.9g), want (%.9g, %.9g)",
          c[0], c[1], c[2], c[3], got[0], got[1], want[0], want[1]);
    CHECK(depth_key(a) == depth_key(want[0]) && depth_key(b) == depth_key(want[1]), "the reference writes the used range back");
    ref(c[0], c[1], nullptr, nullptr, want);
    depth_range_smooth(c[0], c[1], false, prev, got);
    CHECK(got[0] == c[0] && got[1] == c[1] && want[0] == c[0] && want[1] == c[1], "no previous range");
  }
  const float I[] = {0.f, 100.f, 255.f, 283.3f, 283.4f, 300.f, 1e9f, 1.2f, -10.f};
  const int want[] = {0, 90, 229, 254, 255, 255, 255, 1, 247};
  for (int i = 0; i < 9; i++) CHECK(depth_background(I[i]) == want[i], "background(%g) = %d, want %d", I[i], depth_background(I[i]), want[i]);
  CHECK(depth_background(nan) == 0, "NaN intensity");
  CHECK(depth_background(std::numeric_limits<float>::infinity()) == 0 && depth_background(1e20f) == 0, "a product outside int converts to INT_MIN, low byte 0");
}

int main() {
  test_ring();
  test_gather();
  test_jet();
  test_select();
  test_smooth_background();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("depth_image ok\n");
  return 0;
}
