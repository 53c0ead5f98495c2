// The yardstick of tools/time_depth_image.py: CoarseTracker::debugPlotIDepthMap (CoarseTracker.cpp:1071-1176) restated for one thread of a
// CPU, as the reference runs it: collect the positive pixels, std::sort, the two order statistics, the smoothing, the grey background,
// then one ring of 40 pixels per qualifying pixel in raster order.  The per-pixel statements are those of csrc/depth_image.h, so the
// bytes can be compared with the device's.  Built by the tool with g++ -O3 -ffp-contract=off; no part of the library.
#include "../stereo-dso-g2o_amd/csrc/depth_image.h"
#include <algorithm>
#include <vector>

using namespace sdso;

extern "C" int depth_image_cpu(const float* idepth, const float* dI /* w*h pixels {I, dx, dy} */, int w, int h, float* minID_pt, float* maxID_pt,
                               unsigned char* rgb /* w*h*3 */, int* counts) {
  std::vector<float> allID;
  for (int i = 0; i < h * w; i++)
    if (idepth[i] > 0) allID.push_back(idepth[i]);
  if (allID.empty()) return 1;
  std::sort(allID.begin(), allID.end());
  const int n = (int)allID.size() - 1;
  const float minID_new = allID[(int)(n * 0.05)], maxID_new = allID[(int)(n * 0.95)];
  const bool both = minID_pt != 0 && maxID_pt != 0;
  const float prev[2] = {both ? *minID_pt : 0.f, both ? *maxID_pt : 0.f};
  float used[2];
  depth_range_smooth(minID_new, maxID_new, both, prev, used);
  if (both) { *minID_pt = used[0]; *maxID_pt = used[1]; }
  const float minID = used[0], maxID = used[1];
  for (int i = 0; i < h * w; i++) {
    const unsigned char c = depth_background(dI[3 * (size_t)i]);
    rgb[3 * (size_t)i] = c; rgb[3 * (size_t)i + 1] = c; rgb[3 * (size_t)i + 2] = c;
  }
  int circles = 0;
  const int wl = w;
  for (int y = 3; y < h - 3; y++)
    for (int x = 3; x < wl - 3; x++) {
      const float* bp = idepth + x + y * wl;
      Rgb8 col;
      if (!depth_source(bp[0], bp[1], bp[-1], bp[wl], bp[-wl], minID, maxID, &col)) continue;
      circles++;
      auto set = [&](int u, int v) { unsigned char* p = rgb + 3 * ((size_t)u + (size_t)v * wl); p[0] = col.c[0]; p[1] = col.c[1]; p[2] = col.c[2]; };
      for (int i = -3; i <= 3; i++) {   // setPixelCirc
        set(x + 3, y + i); set(x - 3, y + i); set(x + 2, y + i); set(x - 2, y + i);
        set(x + i, y - 3); set(x + i, y + 3); set(x + i, y - 2); set(x + i, y + 2);
      }
    }
  counts[0] = (int)allID.size(); counts[1] = circles;
  return 0;
}
