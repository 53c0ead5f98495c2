// The RawResidualJacobian on the device and what reads it, stated once for every BA kernel (ba_lin / ba_state / ba_top / ba_sc):
//   the record layout   j_off (ba_kernels.h), J_* / jdev / JV, load_J_group / load_J
//   rules on a record   jac_delta (J * delta of EFResidual::fixLinearizationF and calcLEnergyPt), JAC_TAKE_DATA (EFResidual::takeDataF)
//   the tiled sampler   tile0_px, interp33_tiled (getInterpolatedElement33 on 12-byte pixels in 5x2 tiles)
//   block_sum_d         the f64 block sum of the energy partials
#pragma once
#include "ba_kernels.h"

namespace sdso {

// Device layout of one RawResidualJacobian: 19 float4 groups (76 floats; group g of residual i at J + j_off(S, i, g), ba_kernels.h:
// blocks of 64 residuals x 19 groups), ordered so that linearize can store every group as soon as it is known:
//   g0..g2 Jpdxi[0][0..5],Jpdxi[1][0..5] | g3 Jpdc[0] | g4 Jpdc[1] | g5 {Jpdd[0],Jpdd[1],-,-}
//   g6+k {resF[k], JIdx[0][k], JIdx[1][k], JabF[0][k]} k=0..7 | g14,g15 JabF[1][0..7] | g16 JIdx2 | g17 JabJIdx | g18 Jab2
// group g of residual i -> jl[4 g .. 4 g + 3]
__device__ __forceinline__ void load_J_group(const float* J, int S, int i, int g, float* jl) {
  const float4 q = *(const float4*)(J + j_off(S, i, g));
  jl[4 * g] = q.x; jl[4 * g + 1] = q.y; jl[4 * g + 2] = q.z; jl[4 * g + 3] = q.w;
}
__device__ __forceinline__ void load_J(const float* J, int S, int i, float* jl) {
#pragma unroll
  for (int g = 0; g < 19; g++) load_J_group(J, S, i, g, jl);
}
// first ABI field (include/sdso_abi.h order) of every member of the record
constexpr int J_RESF = 0, J_XI0 = 8, J_XI1 = 14, J_C0 = 20, J_C1 = 24, J_DD = 28, J_IDX0 = 30, J_IDX1 = 38, J_AB0 = 46, J_AB1 = 54,
              J_IDX2 = 62, J_ABIDX = 66, J_AB2 = 70;
// ABI field index (include/sdso_abi.h order) -> index in the device layout
__host__ __device__ constexpr int jdev(int f) {
  return f < 8 ? 24 + 4 * f : f < 14 ? (f - 8) : f < 20 ? 6 + (f - 14) : f < 24 ? 12 + (f - 20) : f < 28 ? 16 + (f - 24) : f < 30 ? 20 + (f - 28)
       : f < 38 ? 24 + 4 * (f - 30) + 1 : f < 46 ? 24 + 4 * (f - 38) + 2 : f < 54 ? 24 + 4 * (f - 46) + 3 : f < 62 ? 56 + (f - 54)
       : f < 66 ? 64 + (f - 62) : f < 70 ? 68 + (f - 66) : 72 + (f - 70);
}
#define JV(f) jl[jdev(f)]   // (jl: a record in registers, device layout)

// The image-space part of J * delta: dx, dy of EFResidual::fixLinearizationF (EnergyFunctionalStructs.cpp:96-123) and
// EnergyFunctional::calcLEnergyPt (EnergyFunctional.cpp:354-417).  dp = adHTdeltaF of the pair (its [6], [7] are the caller's affine
// terms), dc = cDeltaF, dd = the point's deltaF
__device__ __forceinline__ void jac_delta(const float* jl, const float* dp, const float* dc, float dd, float& dx, float& dy) {
  float sx = 0, sy = 0, cx = 0, cy = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) { sx += JV(J_XI0 + k) * dp[k]; sy += JV(J_XI1 + k) * dp[k]; }
#pragma unroll
  for (int k = 0; k < 4; k++) { cx += JV(J_C0 + k) * dc[k]; cy += JV(J_C1 + k) * dc[k]; }
  dx = sx + cx + JV(J_DD + 0) * dd;
  dy = sy + cy + JV(J_DD + 1) * dd;
}
// EFResidual::takeDataF (EnergyFunctionalStructs.cpp:37-51): JpJdF[8] -> out from groups 0, 1, 2, 5, 16, 17 of the caller's jl (a macro for
// the reason given in ba_lin.hip: k_ba_lin_fused's listing)
constexpr int kTakeDataGroups[6] = {0, 1, 2, 5, 16, 17};
#define JAC_TAKE_DATA(out)                                                               \
  {                                                                                      \
    const float jdd0 = JV(J_DD + 0), jdd1 = JV(J_DD + 1);                                \
    const float v0 = JV(J_IDX2 + 0) * jdd0 + JV(J_IDX2 + 1) * jdd1;                      \
    const float v1 = JV(J_IDX2 + 2) * jdd0 + JV(J_IDX2 + 3) * jdd1;                      \
    _Pragma("unroll")                                                                    \
    for (int k = 0; k < 6; k++) out[k] = JV(J_XI0 + k) * v0 + JV(J_XI1 + k) * v1;        \
    out[6] = JV(J_ABIDX + 0) * jdd0 + JV(J_ABIDX + 1) * jdd1;                            \
    out[7] = JV(J_ABIDX + 2) * jdd0 + JV(J_ABIDX + 3) * jdd1;                            \
  }

// getInterpolatedElement33 on the tiled level-0 image (12-byte pixels in 5x2 tiles, tile0_layout.h): the four taps of a sample and the
// samples of one 8-pixel pattern fall into fewer 128-B lines than in the row-major float4 image (5.7 instead of 8.3 per residual
// on average; 16-byte pixels in 4x2 tiles: 6.25-6.4; profiles/lin_tiles_ab.txt), the arithmetic is the same expression as interp33
struct tile0_px { float x, y, z; };
__device__ __forceinline__ tile0_px tile0_load(const char* __restrict__ img, int x, int y, int T) { return *(const tile0_px*)(img + tile0_offset(x, y, T)); }
__device__ __forceinline__ float3 interp33_tiled(const char* __restrict__ img, float x, float y, int T) {
  const int ix = (int)x;
  const int iy = (int)y;
  const float dx = x - ix;
  const float dy = y - iy;
  const float dxdy = dx * dy;
  const tile0_px p00 = tile0_load(img, ix, iy, T), p10 = tile0_load(img, ix + 1, iy, T), p01 = tile0_load(img, ix, iy + 1, T),
                 p11 = tile0_load(img, ix + 1, iy + 1, T);
  const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
  float3 r;
  r.x = w11 * p11.x + w01 * p01.x + w10 * p10.x + w00 * p00.x;
  r.y = w11 * p11.y + w01 * p01.y + w10 * p10.y + w00 * p00.y;
  r.z = w11 * p11.z + w01 * p01.z + w10 * p10.z + w00 * p00.z;
  return r;
}

__device__ __forceinline__ double block_sum_d(double v, double* lds) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) lds[wv] = v;
  __syncthreads();
  double s = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += lds[w];
  __syncthreads();
  return s;
}

}  // namespace sdso
