// The x transforms and the output rounding shared by the decode GEMMs (skinny_gemm.hip, decode_gemm.hip): the rounding points of the
// fused RMSNorm / SwiGLU and of the residual add are written once, here, so that every kernel stays bit-identical to
// vq3_rmsnorm_fwd / vq3_silu_mul_fwd feeding the plain product.
#pragma once
#include "common.h"

// SwiGLU of 8 gate values f with the 8 up values of upv
__device__ __forceinline__ void swiglu8(float* f, const u32x4 upv) {
  float up[8];
  unpack8(upv, up);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = rbf(rbf(silu_f(f[j])) * up[j]);
}
// 8 elements of row xr at k, SwiGLU applied where XMODE == 2
template <int XMODE>
__device__ __forceinline__ void load_x8(const bf16_t* xr, int k, int K, float* f) {
  unpack8(*(const u32x4*)(xr + k), f);
  if (XMODE == 2) swiglu8(f, *(const u32x4*)(xr + K + k));
}
__device__ __forceinline__ float sumsq8(const float* f, float ss) {
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = fmaf(f[j], f[j], ss);
  return ss;
}
__device__ __forceinline__ void rmsnorm8(float* f, const u32x4 lwv, float rstd) {
  float lw[8];
  unpack8(lwv, lw);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = rbf(lw[j] * rbf(f[j] * rstd));
}
// RESCALED: v is the bf16-valued, rescaled product of the e4m3 path; else the GEMM output becomes bf16 before the residual add
template <bool RESCALED>
__device__ __forceinline__ void store_out(void* y, const bf16_t* res, float v, int m, int n, long ldy, long ldr, int out_f32) {
  if (res) v = (RESCALED ? v : rbf(v)) + bf2f(res[(long)m * ldr + n]);
  if (out_f32) ((float*)y)[(long)m * ldy + n] = v;
  else ((bf16_t*)y)[(long)m * ldy + n] = f2bf(v);
}
