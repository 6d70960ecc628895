// Device helpers shared by the fused Qwen3 attention kernels (head_dim 128, MFMA 32x32x16 bf16, one wave per 32-row block):
// qwen_flash.hip (forward / backward over a [B, H, L, 128] sequence) and qwen_append.hip (a chunk of new positions against the
// resident KV cache). Operand fragments, the 8-byte "transposed" gather, the L2 touch of the next tile and the LDS output tile.
#pragma once
#include "common.h"

namespace {

constexpr int D = 128;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int rho(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int s) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(v[8 * s + j]);
  return o;
}
// Gather of the A operand of "X^T . (acc)" for all four d-blocks: row key(j) contributes 4 consecutive bf16 at column 4r.
// Done in two phases so the loads can be issued a whole tile ahead of their use.
__device__ __forceinline__ void gather_load(const bf16_t* base, long rowstride, int row0, int h, int r, int maxrow,
                                            u32x2 (&g)[2][8]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = row0 + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
      row = row < maxrow ? row : maxrow;
      g[s][j] = *reinterpret_cast<const u32x2*>(base + (long)row * rowstride + 4 * r);
    }
}
__device__ __forceinline__ void gather_split(const u32x2 (&g)[8], bf16x8 (&a)[4]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[0][j] = (short)(g[j][0] & 0xffff);
    a[1][j] = (short)(g[j][0] >> 16);
    a[2][j] = (short)(g[j][1] & 0xffff);
    a[3][j] = (short)(g[j][1] >> 16);
  }
}
__device__ __forceinline__ void rows_load(const bf16_t* base, long rowstride, int row, int h, int maxrow, bf16x8 (&f)[8]) {
  const bf16_t* p = base + (long)(row < maxrow ? row : maxrow) * rowstride + 8 * h;
#pragma unroll
  for (int t = 0; t < 8; ++t) f[t] = ld8(p + 16 * t);
}
// One dword per 128-byte line of a 32-row x 256-byte tile (64 lanes = its 64 lines): pulls the NEXT tile of the walk into this
// XCD's L2 a whole tile ahead, so that its real loads are L2 hits instead of a ~2 us cross-XCD round trip. Costs one register.
__device__ __forceinline__ unsigned touch_tile(const bf16_t* base, long rowstride, int row0, int maxrow) {
  const int lane = threadIdx.x & 63;
  int row = row0 + (lane >> 1);
  row = row < maxrow ? row : maxrow;
  return *reinterpret_cast<const unsigned*>(base + (long)row * rowstride + (lane & 1) * 64);
}

// Output tiles leave through LDS as whole rows. The accumulator layout gives a lane 8-byte pieces (4 features) of ONE row, 16 of them
// 16 bytes apart in pairs: stored straight from registers every store instruction scatters 64 pieces over 32 rows - 1 024 partial-line
// write requests per 8-KiB tile, and for these short kernels the request rate of the L2 write path is what they wait for. put: the
// piece goes to the wave's 8-KiB tile (32 rows x 256 B, 16-byte chunks XOR (row & 15)); flush: 8 passes of 4 whole rows, 16 B per lane.
__device__ __forceinline__ void tile_put8(char* tile, int row, int piece, const u32x2& w) {      // piece = feature / 4
  *reinterpret_cast<u32x2*>(tile + row * 256 + (((piece >> 1) ^ (row & 15)) << 4) + ((piece & 1) << 3)) = w;
}
__device__ __forceinline__ void tile_flush(const char* tile, bf16_t* base, long rowstride, int row0, int L, int lane) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = 4 * p + (lane >> 4);
    const int phys = lane & 15, logical = phys ^ (row & 15);
    const u32x4 v = *reinterpret_cast<const u32x4*>(tile + row * 256 + (phys << 4));
    if (row0 + row < L) *reinterpret_cast<u32x4*>(base + (long)(row0 + row) * rowstride + logical * 8) = v;
  }
}

}  // namespace
