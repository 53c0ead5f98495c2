// Single-thread CPU restatement of the two steps csrc/distmap.hip runs on the device — makeDistanceMap + growDistBFS and the candidate
// loop of activatePointsMT STEP 2 with addIntoDistFinal — timed on the host that drives the GPU (tools/time_distmap.py writes the inputs
// and reads the line this prints).  List-ordered like the reference (two pixel lists swapped per step); not part of the product.
//   distmap_cpu_baseline <dir> <reps>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

template <class T>
static std::vector<T> load(const std::string& dir, const char* name) {
  std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
  if (!f) { std::fprintf(stderr, "missing %s\n", name); std::exit(2); }
  f.seekg(0, std::ios::end);
  const size_t bytes = (size_t)f.tellg();
  f.seekg(0);
  std::vector<T> v(bytes / sizeof(T));
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  return v;
}

struct Map {
  int w1, h1;
  std::vector<float> d;
  std::vector<int> l1, l2;     // pixel lists, x | y << 16
  void grow(int num) {
    for (int k = 1; k < 40; k++) {
      const int num2 = num;
      std::swap(l1, l2);
      num = 0;
      const int nd = (k % 2 == 0) ? 4 : 8;
      static const int DX[8] = {1, -1, 0, 0, 1, -1, -1, 1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
      for (int i = 0; i < num2; i++) {
        const int x = l2[i] & 0xffff, y = l2[i] >> 16;
        if (x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1) continue;
        const int idx = x + y * w1;
        for (int j = 0; j < nd; j++) {
          const int q = idx + DX[j] + DY[j] * w1;
          if (d[q] > k) { d[q] = (float)k; l1[num++] = (x + DX[j]) | ((y + DY[j]) << 16); }
        }
      }
      if (!num) break;
    }
  }
  void add(int u, int v) { l1[0] = u | (v << 16); d[u + w1 * v] = 0; grow(1); }
};

static inline bool project(const float* g, float u, float v, float id, int w1, int h1, int& iu, int& iv, float& p0) {
  p0 = ((g[0] * u + g[1] * v) + g[2]) + g[9] * id;
  const float p1 = ((g[3] * u + g[4] * v) + g[5]) + g[10] * id, p2 = ((g[6] * u + g[7] * v) + g[8]) + g[11] * id;
  const float qx = p0 / p2 + 0.5f, qy = p1 / p2 + 0.5f;
  if (!(std::fabs(qx) < 2e9f && std::fabs(qy) < 2e9f)) return false;
  iu = (int)qx; iv = (int)qy;
  return iu > 0 && iv > 0 && iu < w1 && iv < h1;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: distmap_cpu_baseline <dir> <reps>\n"); return 2; }
  const std::string dir = argv[1];
  const int reps = std::atoi(argv[2]);
  const auto meta = load<int>(dir, "meta");     // w h
  const auto geom = load<float>(dir, "geom");   // ng * 12
  const auto flagged = load<uint8_t>(dir, "flagged");
  const auto a_pg = load<int>(dir, "a_pg");
  const auto a_u = load<float>(dir, "a_u"), a_v = load<float>(dir, "a_v"), a_id = load<float>(dir, "a_idepth");
  const auto c_pg = load<int>(dir, "c_pg");
  const auto c_st = load<uint8_t>(dir, "c_status");
  const auto c_u = load<float>(dir, "c_u"), c_v = load<float>(dir, "c_v"), c_min = load<float>(dir, "c_idepth_min"), c_max = load<float>(dir, "c_idepth_max"),
             c_q = load<float>(dir, "c_quality"), c_itv = load<float>(dir, "c_interval"), c_ty = load<float>(dir, "c_my_type");
  const auto par = load<float>(dir, "par");
  const int w1 = meta[0] >> 1, h1 = meta[1] >> 1, na = (int)a_u.size(), nc = (int)c_u.size();
  Map M{w1, h1, std::vector<float>((size_t)w1 * h1), std::vector<int>((size_t)w1 * h1 + na), std::vector<int>((size_t)w1 * h1 + na)};
  std::vector<double> t_make, t_sel;
  std::vector<uint8_t> dec(nc);
  int n_seeds = 0, n_sel = 0;
  for (int r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    std::fill(M.d.begin(), M.d.end(), 1000.f);
    n_seeds = 0;
    for (int i = 0; i < na; i++) {
      int iu, iv; float p0;
      if (!project(&geom[12 * a_pg[i]], a_u[i], a_v[i], a_id[i], w1, h1, iu, iv, p0)) continue;
      M.d[iu + w1 * iv] = 0;
      M.l1[n_seeds++] = iu | (iv << 16);
    }
    M.grow(n_seeds);
    auto t1 = std::chrono::steady_clock::now();
    n_sel = 0;
    for (int i = 0; i < nc; i++) {
      const uint8_t st = c_st[i];
      if (!std::isfinite(c_max[i]) || st == 2) { dec[i] = 1; continue; }
      const bool can = (st == 0 || st == 3 || st == 4 || st == 1) && c_itv[i] < 8 && c_q[i] > par[1] && (c_max[i] + c_min[i]) > 0;
      if (!can) { dec[i] = (flagged[c_pg[i]] || st == 1) ? 1 : 0; continue; }
      int iu, iv; float p0;
      if (project(&geom[12 * c_pg[i]], c_u[i], c_v[i], 0.5f * (c_max[i] + c_min[i]), w1, h1, iu, iv, p0)) {
        const float dist = M.d[iu + w1 * iv] + (p0 - floorf(p0));
        if (dist >= par[0] * c_ty[i]) { M.add(iu, iv); dec[i] = 2; n_sel++; } else dec[i] = 0;
      } else dec[i] = 1;
    }
    auto t2 = std::chrono::steady_clock::now();
    t_make.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    t_sel.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
  }
  std::sort(t_make.begin(), t_make.end());
  std::sort(t_sel.begin(), t_sel.end());
  unsigned long long hsh = 1469598103934665603ull;
  for (int i = 0; i < nc; i++) hsh = (hsh ^ dec[i]) * 1099511628211ull;
  double msum = 0;
  for (float x : M.d) msum += x;
  std::printf("{\"n_seeds\": %d, \"n_selected\": %d, \"make_us_median\": %.1f, \"make_us_min\": %.1f, \"select_us_median\": %.1f, \"select_us_min\": %.1f, "
              "\"decision_fnv\": %llu, \"final_map_sum\": %.0f}\n",
              n_seeds, n_sel, t_make[t_make.size() / 2], t_make[0], t_sel[t_sel.size() / 2], t_sel[0], hsh, msum);
  return 0;
}
