// The yardstick of tools/time_map_cloud.py: KeyFrameDisplay::setFromKF (IOWrapper/Pangolin/KeyFrameDisplay.cpp:85-165) and refreshPC
// (:174-295) restated from scratch for one thread of a CPU, as the reference runs them: copy the lists of a keyframe into
// InputPointSparse records, then walk them with the keep tests and write 8 vertices and colours per kept point.  z = depth and no
// sparsification, as in the library (its two stated deviations), so the bytes can be compared with the device's.  Built by the tool
// with g++ -O3 -ffp-contract=off; no part of the library and none of its headers.
#include <cstddef>
#include <vector>

namespace {
struct InputPointSparse { float u, v, idpeth, idepth_hessian, relObsBaseline; int numGoodRes; float color[8]; unsigned char status; };
const int patternP[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};
}

// One keyframe.  The caller's points: n records of 16 floats {u, v, idepth, idepth_hessian, maxRelBaseline, color[8], -, -, -} with their
// status (1 active, 2 marginalised, 3 out), in list order — what the PointHessians of fh hold.  Returns the number of vertices.
extern "C" int map_cloud_cpu(int n, const float* rec, const unsigned char* status, float fx, float fy, float cx, float cy, float scaledTH, float absTH,
                             float minBS, int mode, float* xyz, unsigned char* rgb) {
  // ---- setFromKF
  const float fxi = 1 / fx, fyi = 1 / fy, cxi = -cx / fx, cyi = -cy / fy;
  std::vector<InputPointSparse> pc((size_t)n);
  for (int i = 0; i < n; i++) {
    const float* r = rec + (size_t)i * 16;
    for (int k = 0; k < 8; k++) pc[i].color[k] = r[5 + k];
    pc[i].u = r[0]; pc[i].v = r[1]; pc[i].idpeth = r[2]; pc[i].relObsBaseline = r[4]; pc[i].idepth_hessian = r[3]; pc[i].numGoodRes = 0; pc[i].status = status[i];
  }
  // ---- refreshPC
  int nv = 0;
  for (int i = 0; i < n; i++) {
    if (mode == 1 && pc[i].status != 1 && pc[i].status != 2) continue;
    if (mode == 2 && pc[i].status != 1) continue;
    if (mode > 2) continue;
    if (pc[i].idpeth < 0) continue;
    float depth = 1.0f / pc[i].idpeth;
    float depth4 = depth * depth;
    depth4 *= depth4;
    float var = (1.0f / (pc[i].idepth_hessian + 0.01));
    if (var * depth4 > scaledTH) continue;
    if (var > absTH) continue;
    if (pc[i].relObsBaseline < minBS) continue;
    for (int pnt = 0; pnt < 8; pnt++) {
      int dx = patternP[pnt][0];
      int dy = patternP[pnt][1];
      float* V = xyz + (size_t)nv * 3;
      unsigned char* C = rgb + (size_t)nv * 3;
      V[0] = ((pc[i].u + dx) * fxi + cxi) * depth;
      V[1] = ((pc[i].v + dy) * fyi + cyi) * depth;
      V[2] = depth;
      if (mode == 0) {
        const int st = pc[i].status;
        C[0] = st == 3 ? 255 : 0; C[1] = (st == 0 || st == 1) ? 255 : 0; C[2] = (st == 0 || st == 2) ? 255 : 0;
      } else {
        C[0] = C[1] = C[2] = (unsigned char)pc[i].color[pnt];
      }
      nv++;
    }
  }
  return nv;
}
