// Single-thread CPU restatement of what the host does per image before sdso_make_pyramid can be called — the two full-image passes of
// Undistort::undistort<unsigned char>: the photometric step (G[raw] * vignetteMapInv) into a float image of the raw size, then the bilinear
// remap of every output pixel in the reference's summation order — timed on the host that drives the GPU (tools/time_ingest.py writes the
// inputs and reads the line this prints).  Not part of the product.
//   undistort_cpu_baseline <dir> <reps>       meta = wOrg hOrg w h; raw0 raw1 (uint8), G (256), vinv, remapX, remapY
#include <algorithm>
#include <chrono>
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

// step 1, PhotometricUndistorter::processFrame in mode 2: the response of every raw pixel, then the inverse vignette over the result
static void photometric(const uint8_t* raw, const float* G, const float* vinv, size_t n, float* photo) {
  for (size_t i = 0; i < n; i++) photo[i] = G[raw[i]];
  for (size_t i = 0; i < n; i++) photo[i] *= vinv[i];
}

// step 2: every output pixel blends the four photometric pixels around its remap entry; a negative entry is outside and gives 0.
// The weights are summed lower-right, lower-left, upper-right, upper-left, as the library's kernel and tests/undistort_ref.py do.
static void remap(const float* photo, int wOrg, const float* remapX, const float* remapY, int w, int h, float* out) {
  for (int y = 0; y < h; y++) {
    const float* mx = remapX + (size_t)y * w;
    const float* my = remapY + (size_t)y * w;
    float* o = out + (size_t)y * w;
    for (int x = 0; x < w; x++) {
      if (mx[x] < 0) { o[x] = 0; continue; }
      const int col = (int)mx[x], row = (int)my[x];
      const float fx = mx[x] - col, fy = my[x] - row, fxy = fx * fy;
      const float* up = photo + (size_t)row * wOrg + col;
      const float* down = up + wOrg;
      o[x] = fxy * down[1] + (fy - fxy) * down[0] + (fx - fxy) * up[1] + (1 - fx - fy + fxy) * up[0];
    }
  }
}

static void undistort(const uint8_t* raw, const float* G, const float* vinv, const float* remapX, const float* remapY, int wOrg, int hOrg, int w, int h,
                      float* photo, float* out) {
  photometric(raw, G, vinv, (size_t)wOrg * hOrg, photo);
  remap(photo, wOrg, remapX, remapY, w, h, out);
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: undistort_cpu_baseline <dir> <reps>\n"); return 2; }
  const std::string dir = argv[1];
  const int reps = std::atoi(argv[2]);
  const auto meta = load<int>(dir, "meta");
  const int wOrg = meta[0], hOrg = meta[1], w = meta[2], h = meta[3];
  const auto raw0 = load<uint8_t>(dir, "raw0"), raw1 = load<uint8_t>(dir, "raw1");
  const auto G = load<float>(dir, "G"), vinv = load<float>(dir, "vinv"), rx = load<float>(dir, "remapX"), ry = load<float>(dir, "remapY");
  std::vector<float> photo((size_t)wOrg * hOrg), out0((size_t)w * h), out1((size_t)w * h);
  std::vector<double> t;
  for (int r = 0; r < reps + 3; r++) {
    const auto a = std::chrono::steady_clock::now();
    undistort(raw0.data(), G.data(), vinv.data(), rx.data(), ry.data(), wOrg, hOrg, w, h, photo.data(), out0.data());
    undistort(raw1.data(), G.data(), vinv.data(), rx.data(), ry.data(), wOrg, hOrg, w, h, photo.data(), out1.data());
    const auto b = std::chrono::steady_clock::now();
    if (r >= 3) t.push_back(std::chrono::duration<double, std::micro>(b - a).count());
  }
  std::sort(t.begin(), t.end());
  double sum = 0;
  for (float v : out0) sum += v;
  for (float v : out1) sum += v;
  std::printf("{\"median_us\": %.1f, \"min_us\": %.1f, \"p90_us\": %.1f, \"checksum\": %.9g}\n", t[t.size() / 2], t[0], t[(9 * t.size()) / 10], sum);
  return 0;
}
