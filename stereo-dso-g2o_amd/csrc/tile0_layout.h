// The tiled copy of a level-0 image that the BA linearisation samples (PyramidDev::tiled0): 12-byte pixels {I, dx, dy} in tiles of
// 5 x 2 pixels, one 128-byte line per tile (two rows of 60 bytes, the last 8 bytes unused and zero).  One definition for the producer
// (ctx.hip), the consumers (ba_jac.h, ba_lin.hip), the upload's size check (ba_window.hip) and tests/test_tile_layout_cpu.py.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace sdso {

constexpr int TILE0_W = 5, TILE0_H = 2, TILE0_PIXEL_BYTES = 12, TILE0_ROW_BYTES = TILE0_W * TILE0_PIXEL_BYTES, TILE0_LINE_BYTES = 128;
// A window's images are read through a buffer descriptor of 2 GiB with 32-bit offsets (ba_lin.hip: TAP_RANGE), so its upload refuses
// a tiled copy of TILE0_MAX_BYTES or more.  A pyramid level is at least 8 rows (four tile rows), which bounds the width of an accepted image:
constexpr size_t TILE0_MAX_BYTES = (size_t)1 << 31;
constexpr int TILE0_MAX_W = TILE0_W * (int)(TILE0_MAX_BYTES / TILE0_LINE_BYTES / 4 - 1);   // 20 971 515

// x / 5 as a multiply-shift (one v_mul_hi_u32 and a shift): exact for every x < 2^32, so for every x <= TILE0_MAX_W
__host__ __device__ inline unsigned tile0_div5(unsigned x) { return (unsigned)(((unsigned long long)x * 0xCCCCCCCDull) >> 34); }
__host__ __device__ inline unsigned tile0_mod5(unsigned x) { return x - 5u * tile0_div5(x); }
__host__ __device__ inline int tile0_tiles_per_row(int w) { return (w + TILE0_W - 1) / TILE0_W; }
__host__ __device__ inline int tile0_tile_rows(int h) { return (h + TILE0_H - 1) / TILE0_H; }
// bytes of the tiled copy of a w x h image (what ensure_tiled0 allocates)
__host__ __device__ inline size_t tile0_bytes(int w, int h) { return (size_t)TILE0_LINE_BYTES * (size_t)tile0_tiles_per_row(w) * (size_t)tile0_tile_rows(h); }
// byte offset of pixel (x, y) in a tiled image with T tiles per row:
//   ((y >> 1) * T + x / 5) * 128 + (y & 1) * 60 + (x % 5) * 12,   written as 12 x + 68 (x / 5) + ... (the same number, fewer operations)
__host__ __device__ inline unsigned tile0_offset(int x, int y, int T) {
  return ((unsigned)(y >> 1) * (unsigned)T) * (unsigned)TILE0_LINE_BYTES + (unsigned)(y & 1) * (unsigned)TILE0_ROW_BYTES
       + (unsigned)x * (unsigned)TILE0_PIXEL_BYTES + tile0_div5((unsigned)x) * (unsigned)(TILE0_LINE_BYTES - TILE0_ROW_BYTES);
}

}  // namespace sdso
